"""CPU: the NumPy model of the binary route (tests/binary_model.py) against independent restatements, and the host logic of
the route (``binary_cut``, ``check_binary_shape``, the size / plan functions and the argument errors, which need no device)."""
import ctypes

import numpy as np
import pytest

import binary_model as bm
import rerank_model as rm


def random_bits(rs, n, dim):
    return rs.randint(0, 2 ** 32, (n, dim // 32), dtype=np.uint64).astype(np.uint32)


def unpack(bits):
    """uint32 [..., W] -> bool [..., 32 W], element i = bit i % 32 of dword i / 32."""
    b = np.ascontiguousarray(bits, dtype="<u4")
    return np.unpackbits(b.view(np.uint8), axis=-1, bitorder="little").astype(bool)


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("dim", [128, 384, 768, 4096])
def test_popcount_score_equals_unpackbits(dim):
    rs = np.random.RandomState(dim)
    rows, q = random_bits(rs, 200, dim), random_bits(rs, 1, dim)[0]
    rows[3] = q
    rows[4] = ~q
    s, sim = bm.score(rows, q, dim)
    want = dim - 2 * (unpack(rows) != unpack(q)[None, :]).sum(axis=1)
    assert np.array_equal(s, want) and s.dtype == np.int32
    assert s[3] == dim and s[4] == -dim and sim[3] == 1.0 and sim[4] == -1.0
    assert np.array_equal(sim, (want.astype(np.float64) / dim).astype(np.float32))     # one division, correctly rounded


@pytest.mark.parametrize("dim", [128, 4096])
def test_sim_is_strictly_monotone_in_s(dim):
    s = np.arange(-dim, dim + 1, dtype=np.int32)             # every integer, not only the reachable s = dim (mod 2)
    sim = bm.sim_of(s, dim)
    assert sim.dtype == np.float32 and (np.diff(sim) > 0).all()
    key = rm.ord32(sim).astype(np.int64)
    assert (np.diff(key) > 0).all(), "ord(sim) orders like s"
    assert sim[dim] == 0 and not np.signbit(sim[dim])


def test_bit_layout():
    dim = 256
    for i in (0, 1, 31, 32, 33, 127, 128, 255):
        x = np.full(dim, -1.0, np.float32)
        x[i] = 2.0
        b = bm.binarize(x)
        assert b.shape == (dim // 32,) and b.dtype == np.uint32
        want = np.zeros(dim // 32, np.uint32)
        want[i // 32] = np.uint32(1) << np.uint32(i % 32)
        assert np.array_equal(b, want), i
    rs = np.random.RandomState(0)
    x = rs.randn(7, 3, 384).astype(np.float32)
    assert np.array_equal(unpack(bm.binarize(x)), x > 0)


def test_sign_rule_on_special_values():
    tiny = np.float32(1e-45)                                  # the smallest denormal
    assert tiny > 0 and tiny < np.finfo(np.float32).tiny
    vals = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, tiny, -tiny, np.finfo(np.float32).tiny, 1.0, -1.0], np.float32)
    want = np.array([0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0], bool)
    x = np.zeros(128, np.float32)
    x[: vals.shape[0]] = vals
    assert np.array_equal(unpack(bm.binarize(x))[: vals.shape[0]], want)
    assert not unpack(bm.binarize(x))[vals.shape[0]:].any()
    assert not bm.binarize(np.zeros((2, 128), np.float32)).any(), "an all-zero row: all bits 0"
    assert not bm.binarize(np.full((1, 128), np.nan, np.float32)).any(), "a NaN row: all bits 0"


def test_candidates_order_ties_and_padding():
    dim, n = 128, 300
    rs = np.random.RandomState(1)
    base = random_bits(rs, 5, dim)
    bits = base[rs.randint(0, 5, n)]                          # five distinct rows: every score is shared by dozens
    q = base[:2]
    dewi, ent = rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)
    recs = bm.candidates(bits, q, dewi, ent, 40, id_offset=1000)
    for j in range(2):
        s, sim = bm.score(bits, q[j], dim)
        order = sorted(range(n), key=lambda r: (-int(s[r]), r))[:40]
        assert recs["id"][j].tolist() == [r + 1000 for r in order]
        assert np.array_equal(recs["sim"][j], sim[order]) and np.array_equal(recs["dewi"][j], dewi[order])
        assert np.array_equal(rm.record_order(recs[j]), np.arange(40))
        assert recs["sim"][j, 0] == 1.0
    small = bm.candidates(bits[:3], q, dewi, ent, 8)
    assert (small["id"][:, 3:] == -1).all() and np.isneginf(small["sim"][:, 3:]).all() and (small["id"][:, :3] >= 0).all()


# ------------------------------------------------------------------------------------------------------------ host logic
def test_binary_cut():
    from dewi._engine import binary_cut
    assert binary_cut(10, None, 10 ** 6) == 160
    assert binary_cut(1, None, 10 ** 6) == 128
    assert binary_cut(8, None, 10 ** 6) == 128
    assert binary_cut(9, None, 10 ** 6) == 144
    assert binary_cut(64, None, 10 ** 6) == 1024
    assert binary_cut(100, None, 10 ** 6) == 1024
    assert binary_cut(1024, None, 10 ** 6) == 1024
    assert binary_cut(10, None, 50) == 50
    assert binary_cut(10, 20, 10 ** 6) == 20
    assert binary_cut(10, 1024, 10 ** 6) == 1024
    assert binary_cut(10, 1024, 300) == 300
    assert binary_cut(10, 10, 10 ** 6) == 10
    with pytest.raises(ValueError, match="at most 1024"):
        binary_cut(10, 1025, 10 ** 6)
    with pytest.raises(ValueError, match="exceeds the cut"):
        binary_cut(1025, None, 10 ** 6)
    with pytest.raises(ValueError, match="exceeds the cut"):
        binary_cut(30, 20, 10 ** 6)
    with pytest.raises(ValueError, match="exceeds the cut"):
        binary_cut(10, None, 5)


def test_check_binary_shape():
    from dewi._engine import check_binary_shape
    for dim in (128, 256, 768, 4096):
        check_binary_shape("cosine", False, dim)
    with pytest.raises(ValueError, match="cosine"):
        check_binary_shape("l2", False, 768)
    with pytest.raises(ValueError, match="bf16"):
        check_binary_shape("cosine", True, 768)
    for dim in (0, 64, 127, 192, 1000, 4224, 8192):
        with pytest.raises(ValueError, match="dim % 128"):
            check_binary_shape("cosine", False, dim)


def test_index_switches_need_no_build():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    with pytest.raises(ValueError, match="dim % 128"):
        ExactIndex(192, binary_shadow=True)
    with pytest.raises(ValueError, match="cosine"):
        ExactIndex(128, "l2", binary_shadow=True)
    with pytest.raises(ValueError, match="binary_shadow"):
        IVFIndex(128, binary_shadow=True)
    q = np.zeros(128, np.float32)
    with pytest.raises(ValueError, match="binary_shadow=True"):
        ExactIndex(128).search_binary(q)
    with pytest.raises(ValueError, match="binary_shadow=True"):
        DewiIndex(128, use_ann=False).search_binary(q)
    assert ExactIndex(128, binary_shadow=True, int8_shadow=True, batch_shadow=True)._binary_shadow


# ------------------------------------------------------------------------------------------------------------ the library, no device
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_size_and_plan_need_no_device():
    from dewi import _native as nat
    L = lib()
    assert L.dewi_knn_b1_workspace_bytes(1000, 768, 4, 10) > 0
    for n, dim, b, c in ((0, 768, 1, 10), (1 << 32, 768, 1, 10), (1000, 192, 1, 10), (1000, 64, 1, 10), (1000, 4224, 1, 10),
                         (1000, 768, 0, 10), (1000, 768, 1, 0), (1000, 768, 1, 1025)):
        assert L.dewi_knn_b1_workspace_bytes(n, dim, b, c) == 0, (n, dim, b, c)
    for dim, log2p in ((128, 0), (256, 1), (384, 2), (512, 2), (768, 3), (1024, 3), (2048, 4), (4096, 5)):
        p = nat.b1_plan(5000, dim, 10)
        assert p["log2p"] == log2p and p["rows_per_step"] % (64 >> log2p) == 0 and p["slots"] == 1 and p["n_lists"] == p["blocks"]
    p = nat.b1_plan(5000, 768, 200)
    assert p["slots"] == 4 and p["n_lists"] == 8 * p["blocks"] and p["keys_per_query"] == p["n_lists"] * 200
    p = nat.b1_plan(5000, 768, 1024)
    assert p["slots"] == 0 and p["n_lists"] == 0 and p["keys_per_query"] == 5000
    p = nat.b1_plan(100, 768, 1024)                          # the cut after min(c, n): 100 <= 256 takes lists
    assert p["slots"] == 4 and p["keys_per_query"] == p["n_lists"] * 100
    # the size is the keys of every query, rounded up to 256 bytes
    assert L.dewi_knn_b1_workspace_bytes(5000, 768, 3, 1024) == (3 * 5000 * 8 + 255) // 256 * 256
    with pytest.raises(NotImplementedError):
        nat.b1_plan(1000, 192, 10)


def test_block_cap_of_the_calling_thread():
    from dewi import _native as nat
    L = lib()
    base = nat.b1_plan(1 << 20, 768, 128)
    assert base["slots"] == 4 and base["n_lists"] == 8 * base["blocks"]
    try:
        assert L.dewi_b1_tuning_set(16) == 0
        capped = nat.b1_plan(1 << 20, 768, 128)
        assert capped["blocks"] == min(16, base["blocks"]) and capped["n_lists"] == 8 * capped["blocks"]
        assert capped["keys_per_query"] == capped["n_lists"] * 128
        assert L.dewi_knn_b1_workspace_bytes(1 << 20, 768, 2, 128) == 2 * capped["keys_per_query"] * 8
        assert nat.b1_plan(100, 768, 10)["blocks"] == 1                  # a cap never raises the count
        assert L.dewi_b1_tuning_set(-1) == nat.ERR_INVALID_ARG
    finally:
        assert L.dewi_b1_tuning_set(0) == 0
    assert nat.b1_plan(1 << 20, 768, 128) == base


P = 4096          # a non-null, 16-byte aligned "pointer" that is never dereferenced: every error below precedes device work


@pytest.mark.parametrize("call,code,text", [
    (lambda L: L.dewi_binarize_rows_f32(P, -1, 128, P, None), -1, "n_rows must be positive"),
    (lambda L: L.dewi_binarize_rows_f32(P, 1 << 32, 128, P, None), -5, "exceeds 2^32-1"),
    (lambda L: L.dewi_binarize_rows_f32(P, 10, 0, P, None), -1, "dim must be positive"),
    (lambda L: L.dewi_binarize_rows_f32(P, 10, 192, P, None), -5, "dim % 128 == 0"),
    (lambda L: L.dewi_binarize_rows_f32(P, 10, 4224, P, None), -5, "up to 4096"),
    (lambda L: L.dewi_binarize_rows_f32(None, 10, 128, P, None), -1, "null pointer"),
    (lambda L: L.dewi_binarize_rows_f32(P, 10, 128, None, None), -1, "null pointer"),
    (lambda L: L.dewi_binarize_rows_f32(P + 4, 10, 128, P, None), -1, "16-byte aligned"),
    (lambda L: L.dewi_prepare_queries_b1(P, 0, 128, P, None), -1, "n_queries must be positive"),
    (lambda L: L.dewi_prepare_queries_b1(P, 2, 64, P, None), -5, "dim % 128 == 0"),
    (lambda L: L.dewi_prepare_queries_b1(None, 2, 128, P, None), -1, "null pointer"),
    (lambda L: L.dewi_knn_candidates_b1(None, 10, 128, P, 1, P, P, 5, 0, P, P, 1 << 20, None), -1, "null bits or query"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, None, 1, P, P, 5, 0, P, P, 1 << 20, None), -1, "null bits or query"),
    (lambda L: L.dewi_knn_candidates_b1(P, 0, 128, P, 1, P, P, 5, 0, P, P, 1 << 20, None), -1, "n_rows must be positive"),
    (lambda L: L.dewi_knn_candidates_b1(P, 1 << 32, 128, P, 1, P, P, 5, 0, P, P, 1 << 20, None), -5, "exceeds 2^32-1"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 192, P, 1, P, P, 5, 0, P, P, 1 << 20, None), -5, "dim % 128 == 0"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 8192, P, 1, P, P, 5, 0, P, P, 1 << 20, None), -5, "up to 4096"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 0, P, P, 5, 0, P, P, 1 << 20, None), -1, "n_queries must be positive"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 0, 0, P, P, 1 << 20, None), -1, "n_candidates must be positive"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 1025, 0, P, P, 1 << 20, None), -5, "n_candidates 1025 exceeds"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, None, P, 5, 0, P, P, 1 << 20, None), -1, "null payload or output"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 5, 0, None, P, 1 << 20, None), -1, "null payload or output"),
    (lambda L: L.dewi_knn_candidates_b1(P + 8, 10, 128, P, 1, P, P, 5, 0, P, P, 1 << 20, None), -1, "16-byte aligned"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 5, -1, P, P, 1 << 20, None), -5, "must fit int32"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 5, 2 ** 31 - 5, P, P, 1 << 20, None), -5, "must fit int32"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 5, 0, P, None, 1 << 20, None), -3, "workspace"),
    (lambda L: L.dewi_knn_candidates_b1(P, 10, 128, P, 1, P, P, 5, 0, P, P, 8, None), -3, "workspace 8 B < required"),
    (lambda L: L.dewi_knn_b1_plan(10, 128, 5, None), -1, "null out_words"),
    (lambda L: L.dewi_knn_b1_plan(10, 128, 5000, (ctypes.c_int64 * 6)()), -5, "does not take"),
])
def test_argument_errors_precede_device_work(call, code, text):
    from dewi import _native as nat
    assert call(lib()) == code
    assert text in nat.last_error(), nat.last_error()


def test_zero_rows_binarise_to_nothing():
    assert lib().dewi_binarize_rows_f32(P, 0, 128, P, None) == 0

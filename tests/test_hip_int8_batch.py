"""The int8 batch pass (``dewi_knn_candidates_i8_batch``, include/dewi_hip.h "INT8 batch pass") against ``int8_model``.

The int8 score is defined in exact integers, so there is no tolerance anywhere in this file: the records of the pass equal the
NumPy model's and the row route's (``dewi_knn_candidates_i8``) in every bit.  The model is fed the library's own codes and
prepared queries (both checked against the model by tests/test_hip_int8.py); its ``D`` is formed here with a float64 BLAS
product, exact because ``|D| <= 127^2 * 1536 < 2^53``, and goes through ``int8_model``'s own ``key_sim`` and ordering.

Every call runs in a workspace of exactly the required size between two guards (``wsguard.GuardedBuffer``), poisoned before
the call: a write outside it, or a read of what it held, fails the test that made it.
"""
import numpy as np
import pytest

import int8_model as im
import rerank_model as rm
import wsguard

pytestmark = pytest.mark.gpu

FLOOR = 4096          # smallest corpus the pass takes (csrc/launch.hpp kI8MfmaMinRows)
MIN_B = 2             # smallest batch (kI8MfmaMinQueries)
_cache = {}


def _lib():
    from dewi import _native as nat
    return nat.load_library()


def unit_rows(n, dim, seed):
    x = np.random.RandomState(seed).randn(n, dim)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def payload(n, seed):
    rs = np.random.RandomState(seed + 77)
    return rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)


def planted_rows(n, dim, seed):
    """Gaussian unit rows with a NaN element, an inf element, zero rows, a row on .5 code boundaries and a flat +-max row
    (tests/test_hip_int8.py planted_rows), one of each in the LAST tile too."""
    x = unit_rows(n, dim, seed)
    x[3, dim // 2] = np.nan
    x[9, dim - 1] = -np.inf
    x[17] = 0
    x[25] = 0
    x[25, 0], x[25, 1], x[25, 2], x[25, dim - 1] = 127 / 128, 2.5 / 128, 3.5 / 128, -0.5 / 128
    x[40] = np.float32(0.25) * np.where(np.arange(dim) % 3 == 0, -1, 1)
    x[n - 1, 0] = np.nan
    x[n - 2] = 0
    x[n - 3] = x[40]
    return x


def planted_queries(b, dim, x, seed):
    """Gaussian queries; query 0 is a corpus row, query 1 is zero, query 2 (of three or more) has a NaN element."""
    q = np.random.RandomState(seed).randn(b, dim).astype(np.float32)
    q[0] = x[5]
    q[1] = 0
    if b > 2:
        q[2, dim // 3] = np.nan
    return q


def quantize_dev(E_dev):
    import torch
    from dewi import _native as nat
    n, dim = int(E_dev.shape[0]), int(E_dev.shape[1])
    codes = torch.empty((n, dim), dtype=torch.int8, device="cuda")
    scales = torch.empty(n, dtype=torch.float32, device="cuda")
    nat.check(_lib().dewi_quantize_rows_i8(nat.ptr(E_dev), n, dim, nat.ptr(codes), nat.ptr(scales), nat.stream_ptr()))
    return codes, scales


def prepare_dev(Q_dev):
    """``dewi_prepare_queries_i8`` -> host (codes int8 [B, dim], scales fp32 [B])."""
    import torch
    from dewi import _native as nat
    b, dim = int(Q_dev.shape[0]), int(Q_dev.shape[1])
    codes = torch.empty((b, dim), dtype=torch.int8, device="cuda")
    scales = torch.empty(b, dtype=torch.float32, device="cuda")
    nat.check(_lib().dewi_prepare_queries_i8(nat.ptr(Q_dev), b, dim, nat.ptr(codes), nat.ptr(scales), 0, nat.stream_ptr()))
    torch.cuda.synchronize()
    return codes.cpu().numpy(), scales.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_records_equal(got, want, what):
    for name in ("id", "sim", "dewi", "ent"):
        if not same_bits(got[name], want[name]):
            bad = np.argwhere(np.ascontiguousarray(got[name]).view(np.uint32) != np.ascontiguousarray(want[name]).view(np.uint32))
            q, t = bad[0]
            raise AssertionError(f"{what}: field {name} differs at query {q} position {t} ({bad.shape[0]} places): "
                                 f"got {got[q, t]} want {want[q, t]}")


def model_candidates(row_codes, row_scales, q_codes, q_scales, dewi32, ent32, c, id_offset=0):
    """``int8_model.candidates`` with D from one float64 BLAS product (exact: |D| < 2^53)."""
    n = row_codes.shape[0]
    d = row_codes.astype(np.float64) @ q_codes.astype(np.float64).T                     # [n, B]
    assert np.abs(d).max(initial=0) < 2 ** 31 and np.array_equal(d, np.rint(d))
    out = np.zeros((q_codes.shape[0], c), im.RECORD)
    out["sim"], out["id"] = -np.inf, -1
    rows = np.arange(n)
    for j in range(q_codes.shape[0]):
        with np.errstate(invalid="ignore"):
            s = d[:, j].astype(np.int32).astype(np.float32) * np.asarray(row_scales, np.float32)
            sim = (s * np.float32(q_scales[j])).astype(np.float32)
        order = np.lexsort((rows, -rm.ord32(sim).astype(np.int64)))[: min(c, n)]
        m = order.shape[0]
        out["sim"][j, :m] = im.key_sim(sim[order])
        out["dewi"][j, :m] = dewi32[order]
        out["ent"][j, :m] = ent32[order]
        out["id"][j, :m] = order + id_offset
    return out


def plan(n, dim, b, c):
    from dewi import _native as nat
    return nat.i8_batch_plan(n, dim, b, c)


def batch_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c, id_offset=0, pattern="0xff", n=None, ws=None):
    """``dewi_knn_candidates_i8_batch`` on the first ``n`` rows in a guarded, poisoned workspace of exactly the required size
    -> (records [B, c] on the host, refusal flags uint32 [B], the guarded workspace)."""
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    lib = _lib()
    n = int(codes.shape[0]) if n is None else n
    dim, b = int(codes.shape[1]), int(Q_dev.shape[0])
    need = int(lib.dewi_knn_i8_batch_workspace_bytes(n, dim, b, c))
    assert need > 0, (n, dim, b, c)
    p = plan(n, dim, b, c)
    assert p["total"] == need
    if ws is None:
        ws = wsguard.GuardedBuffer(need, "cuda", pattern, label="batch workspace", seed=c)
    out = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="records")
    nat.check(lib.dewi_knn_candidates_i8_batch(nat.ptr(codes), nat.ptr(scales), n, dim, nat.ptr(Q_dev), b, nat.ptr(dewi_dev),
                                               nat.ptr(ent_dev), c, id_offset, nat.ptr(out.mid), nat.ptr(ws.view), need,
                                               nat.stream_ptr()))
    torch.cuda.synchronize()
    out.check()
    ws.check()
    flags = ws.view[p["flags_off"]: p["flags_off"] + 4 * b].cpu().numpy().view(np.uint32)
    assert np.isin(flags, (0, 1)).all(), flags
    return records_to_numpy(out.mid), flags, ws


def rows_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c, id_offset=0):
    """``dewi_knn_candidates_i8`` (the row passes) -> records on the host."""
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    lib = _lib()
    n, dim, b = int(codes.shape[0]), int(codes.shape[1]), int(Q_dev.shape[0])
    need = int(lib.dewi_knn_i8_workspace_bytes(n, dim, b, c))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((b, c, 4), dtype=torch.int32, device="cuda")
    nat.check(lib.dewi_knn_candidates_i8(nat.ptr(codes), nat.ptr(scales), n, dim, nat.ptr(Q_dev), b, nat.ptr(dewi_dev), nat.ptr(ent_dev),
                                         c, id_offset, nat.ptr(out), nat.ptr(ws), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    return records_to_numpy(out)


# ------------------------------------------------------------------------------------------------------------ 1. lane maps
@pytest.mark.parametrize("dim", [64, 80])
def test_lane_maps_with_exact_integers(dim):
    """Row i holds ONE code, 127 at column (7 i) mod dim, and a scale that is a power of two; query j is a ramp of its own.
    D(i, j) = 127 * code_q[j, (7 i) mod dim]: a row <-> query swap, a wrong k pairing or a wrong accumulator -> row map
    changes the integers."""
    import torch
    n, b, c = FLOOR + 37, 32, 64
    rows = np.arange(n)
    rc = np.zeros((n, dim), np.int8)
    rc[rows, (7 * rows) % dim] = 127
    rsc = np.ldexp(np.float32(1), (rows % 40) - 20).astype(np.float32)                  # 2^-20 .. 2^19, distinct inside a tile
    cols = np.arange(dim)
    q = np.stack([((cols * (2 * j + 1) + 3 * j) % 251 - 125).astype(np.float32) + j for j in range(b)])
    dewi, ent = payload(n, dim)
    Q_dev = torch.from_numpy(q).cuda()
    qc, qs = prepare_dev(Q_dev)
    assert len({qc[j].tobytes() for j in range(b)}) == b
    got, _, _ = batch_dev(torch.from_numpy(rc).cuda(), torch.from_numpy(rsc).cuda(), Q_dev, torch.from_numpy(dewi).cuda(),
                          torch.from_numpy(ent).cuda(), c)
    assert_records_equal(got, model_candidates(rc, rsc, qc, qs, dewi, ent, c), f"lane maps, dim {dim}")


# ------------------------------------------------------------------------------------------------------------ 2. the model
def gaussian_case(dim, n):
    """The planted corpus on the device, its codes on the host, its payload — once per (dim, n)."""
    import torch
    key = ("gauss", dim, n)
    if key not in _cache:
        x = planted_rows(n, dim, 31 * dim + n)
        dewi, ent = payload(n, dim)
        codes, scales = quantize_dev(torch.from_numpy(x).cuda())
        _cache[key] = (x, codes, scales, codes.cpu().numpy(), scales.cpu().numpy(), dewi, ent, torch.from_numpy(dewi).cuda(),
                       torch.from_numpy(ent).cuda())
    return _cache[key]


# (dim, n, B, c, id_offset): every value of every axis of the issue's grid; the c = 20 cases also assert that nothing is refused
MODEL_CASES = [
    (64, FLOOR, MIN_B, 1, 0), (64, FLOOR + 37, 33, 20, 1000), (80, FLOOR + 37, 32, 65, 0), (80, 3 * FLOOR, 64, 256, 0),
    (272, FLOOR, 33, 64, 0), (272, 3 * FLOOR + 5, MIN_B, 20, 0), (768, FLOOR + 37, 32, 20, 0), (768, 3 * FLOOR, 64, 20, 1000),
    (768, FLOOR, 32, 256, 0), (768, 3 * FLOOR, 33, 65, 0), (1536, FLOOR + 37, 32, 20, 0), (1536, 3 * FLOOR, 33, 256, 1000),
    (1536, FLOOR, 64, 1, 0), (1520, FLOOR + 37, MIN_B, 64, 0),
]


@pytest.mark.parametrize("dim,n,b,c,id_offset", MODEL_CASES)
def test_records_equal_the_model(dim, n, b, c, id_offset):
    import torch
    x, codes, scales, rc, rsc, dewi, ent, dewi_dev, ent_dev = gaussian_case(dim, n)
    q = planted_queries(b, dim, x, c + b)
    Q_dev = torch.from_numpy(q).cuda()
    qc, qs = prepare_dev(Q_dev)
    assert qs[1] == 0 and (b < 3 or np.isnan(qs[2]))
    got, flags, _ = batch_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c, id_offset)
    want = model_candidates(rc, rsc, qc, qs, dewi, ent, c, id_offset)
    assert_records_equal(got, want, f"{dim} x {n}, B {b}, c {c}")
    # the zero and the NaN query tie on every row: more survivors than their segments hold -> refused, repaired, rows 0 .. c-1
    p = plan(n, dim, b, c)
    assert n > p["n_seg"] * p["seg_cap"], p
    assert flags[1] == 1 and flags[2:3].all(), flags
    nan_rows = np.flatnonzero(np.isnan(rsc))
    first = np.concatenate([nan_rows, np.setdiff1d(np.arange(n), nan_rows)])[:c]           # query 1: NaN rows first
    assert np.array_equal(got["id"][1] - id_offset, first)
    assert b < 3 or np.array_equal(got["id"][2] - id_offset, np.arange(c))
    if c == 20:     # Gaussian queries: the segments hold several times the expected survivors
        others = np.setdiff1d(np.arange(b), [1, 2])
        assert not flags[others].any(), f"refused Gaussian queries {np.flatnonzero(flags).tolist()} (plan {p})"


# ------------------------------------------------------------------------------------------------------------ 3. refusal and repair
@pytest.mark.parametrize("dim,n,b,c", [(768, FLOOR + 37, 32, 20), (272, 3 * FLOOR, 33, 200), (80, FLOOR, MIN_B, 64)])
def test_a_corpus_of_copies_is_refused_and_repaired(dim, n, b, c):
    """n identical rows but a few: every query's c-th best is the tie, every copy survives, the segments overflow."""
    import torch
    x = unit_rows(n, dim, dim)
    keep = [0, 7, n // 2, n - 1]
    distinct = x[keep].copy()
    x[:] = x[11]
    x[keep] = distinct
    q = np.random.RandomState(n).randn(b, dim).astype(np.float32)
    q[0] = x[11]
    dewi, ent = payload(n, dim)
    E_dev, Q_dev = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    codes, scales = quantize_dev(E_dev)
    p = plan(n, dim, b, c)
    assert n - len(keep) > p["n_seg"] * p["seg_cap"], p                                # the segments MUST overflow
    got, flags, _ = batch_dev(codes, scales, Q_dev, torch.from_numpy(dewi).cuda(), torch.from_numpy(ent).cuda(), c)
    qc, qs = prepare_dev(Q_dev)
    assert_records_equal(got, model_candidates(codes.cpu().numpy(), scales.cpu().numpy(), qc, qs, dewi, ent, c), "copies")
    assert flags.all(), flags
    copies = np.setdiff1d(np.arange(n), keep)
    for j in range(b):                                                                 # the ties come in row order
        ids = got["id"][j]
        tied = ids[np.isin(ids, copies)]
        assert tied.size >= c - len(keep) and np.array_equal(tied, copies[: tied.size]), j


# ------------------------------------------------------------------------------------------------------------ 4. the row route
@pytest.mark.parametrize("kind", ["embedding_like", "planted_runs"])
def test_same_bits_as_the_row_route(kind):
    import torch
    import corpora
    n, dim, b = 200_000, 768, 32
    if kind == "embedding_like":
        x, q = corpora.embedding_like(n, dim, 5, n_queries=b)[:2]
    else:
        x, q = corpora.planted_runs(n, dim, b, 5, d_max=320)[:2]
    dewi, ent = payload(n, 3)
    codes, scales = quantize_dev(torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda())
    Q_dev = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    dewi_dev, ent_dev = torch.from_numpy(dewi).cuda(), torch.from_numpy(ent).cuda()
    for c in (20, 200):
        got, flags, _ = batch_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c)
        assert_records_equal(got, rows_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c), f"{kind}, c {c}")
        print(f"{kind} c={c}: {int(flags.sum())} of {b} queries refused and repaired")


# ------------------------------------------------------------------------------------------------------------ 5. bounds
@pytest.mark.parametrize("dim,n", [(768, FLOOR + 37), (80, FLOOR + 1), (1536, 3 * FLOOR - 31)])
def test_nothing_outside_the_rows_is_scored(dim, n):
    """The codes are the first n rows of a larger tensor whose other rows would win every query (code 127 everywhere, scale
    1e30): the result is that of an exactly sized copy."""
    import torch
    b, c, extra = 33, 20, 200
    x, codes, scales, rc, rsc, dewi, ent, dewi_dev, ent_dev = gaussian_case(dim, n)
    big_codes = torch.full((n + extra, dim), 127, dtype=torch.int8, device="cuda")
    big_scales = torch.full((n + extra,), 1e30, dtype=torch.float32, device="cuda")
    big_codes[:n] = codes
    big_scales[:n] = scales
    Q_dev = torch.from_numpy(np.abs(planted_queries(b, dim, x, n))).cuda()            # positive queries: the extra rows score ~1e30
    exact, _, _ = batch_dev(codes.clone(), scales.clone(), Q_dev, dewi_dev, ent_dev, c)
    got, _, _ = batch_dev(big_codes, big_scales, Q_dev, dewi_dev, ent_dev, c, n=n)
    assert_records_equal(got, exact, f"first {n} rows of {n + extra}")
    assert got["id"].max() < n and not np.any(got["sim"] > 1e20)


# ------------------------------------------------------------------------------------------------------------ 6. workspace
@pytest.mark.parametrize("dim,n,b,c", [(768, FLOOR + 37, 33, 20), (272, 3 * FLOOR, 32, 256)])
def test_workspace_contract(dim, n, b, c):
    """The records do not depend on what the workspace held (0x00, random, 0x7F, 0xFF), nor on an earlier call's leavings."""
    import torch
    x, codes, scales, rc, rsc, dewi, ent, dewi_dev, ent_dev = gaussian_case(dim, n)
    Q_dev = torch.from_numpy(planted_queries(b, dim, x, 3)).cuda()
    base = None
    for pattern in wsguard.PATTERNS:
        got, flags, ws = batch_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c, pattern=pattern)
        again, flags2, _ = batch_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c, ws=ws)         # twice on one workspace
        if base is None:
            base = (got, flags)
        for r, f in ((got, flags), (again, flags2)):
            assert_records_equal(r, base[0], f"pattern {pattern}")
            assert np.array_equal(f, base[1])


# ------------------------------------------------------------------------------------------------------------ 7. Python
def columns(n, seed):
    rs = np.random.RandomState(seed)
    return {"dewi": rs.rand(n), "ht_mean": rs.rand(n), "hi_mean": rs.rand(n)}


def shadowed(cls):
    if ("idx", cls) not in _cache:
        from dewi.backends import ExactIndex
        from dewi.index import DewiIndex
        n, dim = FLOOR + 37, 128                         # (batches of 8 queries or more take the pass by default)
        x = np.random.RandomState(dim).randn(n, dim).astype(np.float32)
        x[50:60] = x[49]
        idx = ExactIndex(dim, int8_shadow=True) if cls == "exact" else DewiIndex(dim, use_ann=False, int8_shadow=True)
        idx.add_batch_columns([f"d{i:06d}" for i in range(n)], x, columns(n, dim))
        idx.build()
        q = np.random.RandomState(dim + 1).randn(33, dim).astype(np.float32)
        q[1] = x[49]
        _cache[("idx", cls)] = (x, q, idx)
    return _cache[("idx", cls)]


@pytest.mark.parametrize("rescore", [True, False])
@pytest.mark.parametrize("b", [32, 33])
def test_search_batch_equals_row_by_row_search(b, rescore):
    x, q, idx = shadowed("exact")
    k = 10
    assert _lib().dewi_knn_i8_batch_workspace_bytes(x.shape[0], x.shape[1], b, 2 * k) > 0       # the batch takes the pass
    rows, scores = idx.search_batch(q[:b], k, 0.3, 0.2, approx=True, rescore=rescore)
    assert any(key[0] == "i8batch" for key in idx._corpus.cached_workspaces())
    for j in range(b):
        one_rows, one_scores = idx.search_batch(q[j: j + 1], k, 0.3, 0.2, approx=True, rescore=rescore)
        assert np.array_equal(rows[j], one_rows[0]), j
        assert same_bits(scores[j], one_scores[0]), j


def test_dewi_index_batch_equals_single_searches():
    x, q, idx = shadowed("dewi")
    res = idx.search_batch(q[:32], 10, approx=True)
    for j in (0, 1, 17, 31):
        assert res[j] == idx.search(q[j], 10, approx=True), j


def test_batch_pass_keyword():
    import torch
    x, q, idx = shadowed("exact")
    corpus = idx._corpus
    Q_dev = torch.from_numpy(q).cuda()
    a = corpus.candidates_i8_device(Q_dev, 20, batch_pass=True)
    b = corpus.candidates_i8_device(Q_dev, 20, batch_pass=False)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    alone = corpus.to_int8()
    for k, cand in ((10, None), (5, 200)):
        on = alone.search_approx(q, k, 0.3, 0.2, cand, rescore=False, batch_pass=True)
        off = alone.search_approx(q, k, 0.3, 0.2, cand, rescore=False, batch_pass=False)
        auto = alone.search_approx(q, k, 0.3, 0.2, cand)
        assert np.array_equal(on[0], off[0]) and same_bits(on[1], off[1])
        assert np.array_equal(on[0], auto[0]) and same_bits(on[1], auto[1])
    # shapes the pass does not take: a cut above 256, one query, dim 48
    with pytest.raises(ValueError, match="batch_pass=True"):
        corpus.candidates_i8_device(Q_dev, 300, batch_pass=True)
    with pytest.raises(ValueError, match="batch_pass=True"):
        corpus.candidates_i8_device(Q_dev[:1], 20, batch_pass=True)
    z = np.zeros(FLOOR)
    narrow = type(corpus).from_host(unit_rows(FLOOR, 48, 1), z, z, z).enable_int8_shadow()
    Q48 = torch.from_numpy(unit_rows(8, 48, 2)).cuda()
    with pytest.raises(ValueError, match="batch_pass=True"):
        narrow.candidates_i8_device(Q48, 20, batch_pass=True)
    assert torch.equal(narrow.candidates_i8_device(Q48, 20), narrow.candidates_i8_device(Q48, 20, batch_pass=False))
    torch.cuda.synchronize()


def test_few_queries_over_a_small_corpus_keep_the_row_passes_by_default():
    """The default route (``batch_pass=None``): the pass from ``I8_BATCH_AUTO_MIN_ROWS`` rows or ``I8_BATCH_AUTO_MIN_BATCH``
    queries on, the row passes below both; ``batch_pass=True`` takes the pass wherever the library does.  Same records."""
    import torch
    from dewi._engine import DeviceCorpus, I8_BATCH_AUTO_MIN_BATCH, I8_BATCH_AUTO_MIN_ROWS
    assert FLOOR < I8_BATCH_AUTO_MIN_ROWS and MIN_B < I8_BATCH_AUTO_MIN_BATCH

    def took_pass(corpus, b):
        return any(key[:2] == ("i8batch", b) for key in corpus.cached_workspaces())

    z = np.zeros(FLOOR)
    small = DeviceCorpus.from_host(unit_rows(FLOOR, 128, 3), z, z, z).enable_int8_shadow()
    Q = torch.from_numpy(unit_rows(I8_BATCH_AUTO_MIN_BATCH, 128, 4)).cuda()
    few = Q[: I8_BATCH_AUTO_MIN_BATCH - 1].contiguous()
    auto = small.candidates_i8_device(few, 20)
    assert not took_pass(small, few.shape[0])
    forced = small.candidates_i8_device(few, 20, batch_pass=True)
    assert took_pass(small, few.shape[0]) and torch.equal(auto, forced)
    many = small.candidates_i8_device(Q, 20)
    assert took_pass(small, Q.shape[0]) and torch.equal(many, small.candidates_i8_device(Q, 20, batch_pass=False))
    n = I8_BATCH_AUTO_MIN_ROWS
    z = np.zeros(n)
    large = DeviceCorpus.from_host(unit_rows(n, 64, 5), z, z, z).enable_int8_shadow()
    Q2 = torch.from_numpy(unit_rows(MIN_B, 64, 6)).cuda()
    auto = large.candidates_i8_device(Q2, 20)
    assert took_pass(large, MIN_B) and torch.equal(auto, large.candidates_i8_device(Q2, 20, batch_pass=False))
    torch.cuda.synchronize()

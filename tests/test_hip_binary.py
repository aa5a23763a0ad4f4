"""GPU: the approximate route over a 1-bit copy of the corpus (csrc/knn_scan_b1.hip) against tests/binary_model.py.

The Hamming score is an integer and ``sim`` one IEEE division of two exact values, so everything up to the candidate records
is compared BIT FOR BIT: the codes of stored rows and of queries, then ids, ``sim`` bits, order and padding of the records.
The re-scoring is the int8 route's kernel (fp32 in a fixed order): bit for bit where every order gives the same sum, within
the accumulation bound of tests/test_hip_int8.py otherwise.

Shapes are the smallest that reach every path: 1, 3, 6 and 32 units per row (log2p 0, 2, 3, 5; masked lanes at 3 and 6), one
row, fewer rows than a wave load, a tail shorter than the rows in flight, more than one workgroup (read from the library's
plan), the three list forms (c <= 64, c <= 256, dense) and passes of four queries plus singles.

ACCUMULATION BOUND of the end-to-end check on Gaussian rows (``bound`` there): the re-scoring kernel adds ``dim`` products of a unit
row and a unit query in fp32, so its sim lies within ``dim * 2^-24 * 1.0002`` of the float64 inner product — the figure
test_hip_int8.py::test_rescore_on_unit_rows_within_the_accumulation_bound asserts for the same kernel.  Two rows whose
float64 sims lie further apart than twice that keep their order in fp32; the ids must then be the model's.
"""
import numpy as np
import pytest

import binary_model as bm
import int8_model as im
import wsguard

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_cache = {}


def _lib():
    from dewi import _native as nat
    return nat.load_library()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_records_equal(got, want, what):
    for name in ("id", "sim", "dewi", "ent"):
        if not same_bits(got[name], want[name]):
            bad = np.argwhere(np.ascontiguousarray(got[name]).view(np.uint32) != np.ascontiguousarray(want[name]).view(np.uint32))
            q, t = bad[0]
            raise AssertionError(f"{what}: field {name} differs at query {q} position {t} ({bad.shape[0]} places): "
                                 f"got {got[q, t]} want {want[q, t]}")


def payload(n, seed):
    rs = np.random.RandomState(seed + 77)
    return rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)


def binarize_dev(X_dev, queries=False):
    """``dewi_binarize_rows_f32`` / ``dewi_prepare_queries_b1`` into a guarded output -> device int32 [n, dim / 32]."""
    import torch
    from dewi import _native as nat
    n, dim = int(X_dev.shape[0]), int(X_dev.shape[1])
    out = wsguard.GuardedOutput((n, dim // 32), torch.int32, "cuda", label="bits")
    if queries:
        nat.check(_lib().dewi_prepare_queries_b1(nat.ptr(X_dev), n, dim, nat.ptr(out.mid), nat.stream_ptr()))
    else:
        nat.check(_lib().dewi_binarize_rows_f32(nat.ptr(X_dev), n, dim, nat.ptr(out.mid), nat.stream_ptr()))
    torch.cuda.synchronize()
    out.check_guards()
    return out.mid


def host_bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def candidates_dev(bits_dev, dim, Q_dev, dewi_dev, ent_dev, c, id_offset=0):
    """``dewi_knn_candidates_b1`` in a workspace of exactly the required size -> records [B, c] on the host."""
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    lib = _lib()
    n, b = int(bits_dev.shape[0]), int(Q_dev.shape[0])
    need = int(lib.dewi_knn_b1_workspace_bytes(n, dim, b, c))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="records")
    nat.check(lib.dewi_knn_candidates_b1(nat.ptr(bits_dev), n, dim, nat.ptr(Q_dev), b, nat.ptr(dewi_dev), nat.ptr(ent_dev), c, id_offset,
                                         nat.ptr(out.mid), nat.ptr(ws), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    out.check()
    return records_to_numpy(out.mid.clone())


# ------------------------------------------------------------------------------------------------------------ codes
def planted_rows(n, dim, seed):
    """Gaussian rows (NOT normalised: the sign rule reads raw values) with -0.0, NaN, +-inf, denormals and all-zero rows."""
    x = np.random.RandomState(seed).randn(n, dim).astype(np.float32)
    x[0, :6] = [-0.0, 0.0, np.nan, np.inf, -np.inf, 1e-45]
    x[0, dim - 1] = -1e-45
    if n >= 63:
        x[17] = 0
        x[25] = -0.0
        x[33] = np.nan
        x[40] = np.inf
        x[41] = np.inf
        x[41, ::2] = -np.inf
        x[50] = np.float32(1e-45) * np.where(np.arange(dim) % 3 == 0, -1, 1)
    return x


@pytest.mark.parametrize("n", [1, 63, 1000])
@pytest.mark.parametrize("dim", [128, 384, 768, 4096])
def test_codes_equal_the_model(dim, n):
    import torch
    x = planted_rows(n, dim, dim + n)
    X_dev = torch.from_numpy(x).cuda()
    want = bm.binarize(x)
    assert np.array_equal(host_bits(binarize_dev(X_dev)), want), "dewi_binarize_rows_f32"
    assert np.array_equal(host_bits(binarize_dev(X_dev, queries=True)), want), "dewi_prepare_queries_b1"
    if n >= 63:
        assert not want[[17, 25, 33]].any() and (want[40] == 0xFFFFFFFF).all() and (want[41] == 0xAAAAAAAA).all()


def test_shadow_of_a_corpus_is_the_model_of_its_stored_rows():
    import torch
    from dewi._engine import DeviceCorpus
    n, dim = 1000, 384
    x = np.random.RandomState(3).randn(n, dim).astype(np.float32)
    x[5] = 0                                             # whatever the build stores for a zero row, its bits follow the rule
    z = np.zeros(n)
    corpus = DeviceCorpus.from_host(x, z, z, z, "cosine").enable_binary_shadow()
    torch.cuda.synchronize()
    assert corpus.has_binary_shadow and tuple(corpus.b1_bits.shape) == (n, dim // 32)
    stored = corpus.emb.cpu().numpy()
    assert np.array_equal(host_bits(corpus.b1_bits), bm.binarize(stored))
    assert not host_bits(corpus.b1_bits)[5].any()
    assert np.array_equal(host_bits(corpus.b1_bits)[np.arange(n) != 5], bm.binarize(x)[np.arange(n) != 5]), "a positive norm changes no sign"


# ------------------------------------------------------------------------------------------------------------ candidates
def corpus_rows(kind, n, dim, seed):
    rs = np.random.RandomState(seed)
    if kind == "gauss":
        x = rs.randn(n, dim).astype(np.float32)
        if n >= 63:
            x[11] = 0
            x[12, dim // 2] = np.nan
            x[13] = -x[0]
        return x
    assert kind == "ties"            # a few dozen distinct rows repeated: hundreds of rows share every score
    base = rs.randn(40, dim).astype(np.float32)
    return base[rs.randint(0, 40, n)]


# sizes at which the plan launches more than one workgroup and the rows in flight do not divide the rows (checked below)
MULTI = {128: 20011, 384: 4099, 768: 4099, 4096: 1001}

# (dim, n, c, B, corpus, id_offset): every dim, row count, cut, batch and list form of the grid
CANDIDATE_CASES = [
    (128, 1, 10, 1, "gauss", 0), (128, 63, 64, 4, "gauss", 5), (128, 3000, 1024, 4, "gauss", 0), (128, 20011, 10, 6, "gauss", 0),
    (128, 20011, 200, 1, "gauss", 9), (128, 63, 200, 6, "gauss", 0),
    (384, 1, 1024, 1, "gauss", 0), (384, 63, 200, 6, "gauss", 0), (384, 4099, 64, 1, "gauss", 7), (384, 4099, 200, 4, "gauss", 0),
    (384, 4099, 1024, 6, "gauss", 0), (384, 4099, 10, 4, "gauss", 0),
    (768, 1, 64, 4, "gauss", 0), (768, 63, 10, 1, "gauss", 0), (768, 4099, 10, 4, "gauss", 1000), (768, 4099, 200, 6, "gauss", 0),
    (768, 4099, 1024, 1, "gauss", 3), (768, 4099, 64, 6, "gauss", 0), (768, 63, 1024, 4, "gauss", 0),
    (4096, 1, 10, 1, "gauss", 0), (4096, 63, 64, 6, "gauss", 0), (4096, 1001, 10, 1, "gauss", 0), (4096, 1001, 200, 4, "gauss", 3),
    (4096, 1001, 1024, 1, "gauss", 0), (4096, 1001, 64, 6, "gauss", 0),
    # ties, across waves and workgroups, through every list form
    (128, 20011, 10, 4, "ties", 0), (128, 20011, 64, 1, "ties", 0), (128, 20011, 200, 6, "ties", 2), (128, 20011, 1024, 4, "ties", 0),
]


def test_multi_workgroup_sizes_are_what_the_plan_says():
    from dewi import _native as nat
    for dim, n in MULTI.items():
        for c in (10, 200, 1024):
            p = nat.b1_plan(n, dim, c)
            assert p["blocks"] > 1 and n % p["rows_per_step"] != 0 and n % (p["rows_per_step"] // 8) != 0, (dim, n, c, p)
            assert p["slots"] == {10: 1, 200: 4, 1024: 0}[c]
    assert {nat.b1_plan(100, d, 10)["log2p"] for d in MULTI} == {0, 2, 3, 5}


@pytest.mark.parametrize("dim,n,c,b,kind,id_offset", CANDIDATE_CASES)
def test_candidate_records_equal_the_model(dim, n, c, b, kind, id_offset):
    import torch
    x = corpus_rows(kind, n, dim, 31 * dim + n)
    q = np.random.RandomState(c + b).randn(b, dim).astype(np.float32) * 3
    q[0] = x[0] * np.float32(0.5)
    if b >= 4:
        q[2] = 0                                          # a zero query: every bit 0
        q[3, 1] = np.nan
    dewi, ent = payload(n, dim)
    E_dev, Q_dev = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    bits = binarize_dev(E_dev)
    got = candidates_dev(bits, dim, Q_dev, torch.from_numpy(dewi).cuda(), torch.from_numpy(ent).cuda(), c, id_offset)
    qbits = host_bits(binarize_dev(Q_dev, queries=True))
    assert np.array_equal(qbits, bm.binarize(q))
    want = bm.candidates(host_bits(bits), qbits, dewi, ent, c, id_offset)
    assert_records_equal(got, want, f"{dim} x {n}, c {c}, B {b}, {kind}")
    assert got["sim"][0, 0] == 1.0 and got["id"][0, 0] - id_offset == (0 if kind == "gauss" else np.flatnonzero((x == x[0]).all(axis=1))[0])
    if c > n:
        assert (got["id"][:, n:] == -1).all() and np.isneginf(got["sim"][:, n:]).all() and (got["id"][:, :n] >= 0).all()
    if kind == "ties":
        m = min(c, n)
        shared = np.unique(got["sim"][0, :m], return_counts=True)[1]
        assert shared.max() >= min(m, 100), "hundreds of rows share a score"
        same = got["sim"][:, 1:m] == got["sim"][:, : m - 1]
        assert (got["id"][:, 1:m][same] > got["id"][:, : m - 1][same]).all(), "ties in ascending id order"


# ------------------------------------------------------------------------------------------------------------ workspace contract
@pytest.mark.parametrize("dim,c,b", [(768, 20, 1), (768, 200, 5), (768, 300, 4), (128, 20, 5), (128, 300, 1)])
def test_workspace_contract(dim, c, b):
    """Results do not depend on what the workspace held; nothing outside the workspace or the records is written."""
    import torch
    from dewi._engine import DeviceCorpus
    n = 2100
    z = np.zeros(n)
    x = np.random.RandomState(dim + c).randn(n, dim).astype(np.float32)
    corpus = DeviceCorpus.from_host(x, np.random.RandomState(1).rand(n), z, z).enable_binary_shadow()
    Q_dev = torch.from_numpy(np.random.RandomState(b).randn(b, dim).astype(np.float32)).cuda()
    corpus.candidates_b1_device(Q_dev, c)                       # the cache now holds this shape's workspace
    assert set(corpus.cached_workspaces()) == {("b1", b, c)}
    assert wsguard.guard(corpus) == 1
    base = None
    for pattern in wsguard.PATTERNS:
        wsguard.poison(corpus, pattern, seed=c)
        out = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="records")
        corpus.candidates_b1_device(Q_dev, c, out=out.mid)
        torch.cuda.synchronize()
        out.check()
        wsguard.check(corpus)
        got = (out.mid.clone(),)
        if base is None:
            base = got
        wsguard.assert_bit_equal(got, base, f"pattern {pattern}")
    wsguard.release(corpus)
    from dewi._engine import records_to_numpy
    want = bm.candidates(host_bits(corpus.b1_bits), bm.binarize(Q_dev.cpu().numpy()), corpus.dewi32.cpu().numpy(),
                         corpus.ent32.cpu().numpy(), c)
    assert_records_equal(records_to_numpy(base[0]), want, "guarded workspace")


# ------------------------------------------------------------------------------------------------------------ errors
def test_argument_errors_launch_nothing():
    import torch
    from dewi import _native as nat
    lib = _lib()
    n, dim, b, c = 100, 256, 2, 10
    E = torch.randn(n, dim, device="cuda")
    Q = torch.randn(b, dim, device="cuda")
    pay = torch.rand(n, device="cuda")
    bits = binarize_dev(E)
    need = int(lib.dewi_knn_b1_workspace_bytes(n, dim, b, c))
    ws = wsguard.GuardedBuffer(need, "cuda", "0x7f", label="workspace")
    out = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="records")
    obits = wsguard.GuardedOutput((n, dim // 32), torch.int32, "cuda", label="bits")
    p = nat.ptr
    s = nat.stream_ptr()

    def cand(bits_=p(bits), n_=n, dim_=dim, q_=p(Q), b_=b, dewi_=p(pay), ent_=p(pay), c_=c, off_=0, out_=p(out.mid), ws_=p(ws.view),
             bytes_=need):
        return lib.dewi_knn_candidates_b1(bits_, n_, dim_, q_, b_, dewi_, ent_, c_, off_, out_, ws_, bytes_, s)

    cases = [
        (lambda: cand(bits_=None), nat.ERR_INVALID_ARG, "null bits or query"),
        (lambda: cand(q_=None), nat.ERR_INVALID_ARG, "null bits or query"),
        (lambda: cand(n_=0), nat.ERR_INVALID_ARG, "n_rows must be positive"),
        (lambda: cand(n_=1 << 32), nat.ERR_UNSUPPORTED, "exceeds 2^32-1"),
        (lambda: cand(dim_=0), nat.ERR_INVALID_ARG, "dim must be positive"),
        (lambda: cand(dim_=192), nat.ERR_UNSUPPORTED, "dim % 128 == 0"),
        (lambda: cand(dim_=8192), nat.ERR_UNSUPPORTED, "up to 4096"),
        (lambda: cand(b_=0), nat.ERR_INVALID_ARG, "n_queries must be positive"),
        (lambda: cand(c_=0), nat.ERR_INVALID_ARG, "n_candidates must be positive"),
        (lambda: cand(c_=1025), nat.ERR_UNSUPPORTED, "n_candidates 1025 exceeds"),
        (lambda: cand(dewi_=None), nat.ERR_INVALID_ARG, "null payload or output"),
        (lambda: cand(ent_=None), nat.ERR_INVALID_ARG, "null payload or output"),
        (lambda: cand(out_=None), nat.ERR_INVALID_ARG, "null payload or output"),
        (lambda: cand(bits_=p(bits) + 4), nat.ERR_INVALID_ARG, "16-byte aligned"),
        (lambda: cand(q_=p(Q) + 4), nat.ERR_INVALID_ARG, "16-byte aligned"),
        (lambda: cand(off_=-1), nat.ERR_UNSUPPORTED, "must fit int32"),
        (lambda: cand(off_=2 ** 31 - n), nat.ERR_UNSUPPORTED, "must fit int32"),
        (lambda: cand(ws_=None), nat.ERR_WORKSPACE, "workspace"),
        (lambda: cand(bytes_=need - 1), nat.ERR_WORKSPACE, f"< required {need} B"),
        (lambda: lib.dewi_binarize_rows_f32(None, n, dim, p(obits.mid), s), nat.ERR_INVALID_ARG, "null pointer"),
        (lambda: lib.dewi_binarize_rows_f32(p(E), n, dim, None, s), nat.ERR_INVALID_ARG, "null pointer"),
        (lambda: lib.dewi_binarize_rows_f32(p(E), -3, dim, p(obits.mid), s), nat.ERR_INVALID_ARG, "n_rows must be positive"),
        (lambda: lib.dewi_binarize_rows_f32(p(E), n, 64, p(obits.mid), s), nat.ERR_UNSUPPORTED, "dim % 128 == 0"),
        (lambda: lib.dewi_binarize_rows_f32(p(E) + 4, n, dim, p(obits.mid), s), nat.ERR_INVALID_ARG, "16-byte aligned"),
        (lambda: lib.dewi_prepare_queries_b1(p(Q), 0, dim, p(obits.mid), s), nat.ERR_INVALID_ARG, "n_queries must be positive"),
        (lambda: lib.dewi_prepare_queries_b1(p(Q), b, 4224, p(obits.mid), s), nat.ERR_UNSUPPORTED, "up to 4096"),
        (lambda: lib.dewi_prepare_queries_b1(None, b, dim, p(obits.mid), s), nat.ERR_INVALID_ARG, "null pointer"),
    ]
    for i, (call, code, text) in enumerate(cases):
        assert call() == code, (i, nat.last_error())
        assert text in nat.last_error(), (i, nat.last_error())
    assert lib.dewi_binarize_rows_f32(p(E), 0, dim, p(obits.mid), s) == nat.OK, "no rows: nothing launched"
    torch.cuda.synchronize()
    for t in (out, obits):
        assert bool((t.full.view(torch.uint8) == wsguard.SENTINEL).all()), f"{t.label}: written to by a refused call"
    ws.check(interior=False)
    assert bool((ws.view == 0x7F).all()), "the workspace was written to by a refused call"
    assert cand() == nat.OK                                     # and the same arguments, all valid, run
    torch.cuda.synchronize()
    out.check()


# ------------------------------------------------------------------------------------------------------------ end to end
def columns(n, seed):
    rs = np.random.RandomState(seed)
    return {"dewi": rs.rand(n), "ht_mean": rs.rand(n), "hi_mean": rs.rand(n)}


def build_index(x, cols, cls="exact", **kwargs):
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    ids = [f"d{i:06d}" for i in range(x.shape[0])]
    idx = ExactIndex(x.shape[1], **kwargs) if cls == "exact" else DewiIndex(x.shape[1], use_ann=False, **kwargs)
    idx.add_batch_columns(ids, x, cols)
    idx.build()
    return idx


def exact_dot_rows(n, dim, seed):
    """16 nonzeros of +-0.25 per row, 12 of them in the first 20 columns: unit rows whose inner products are exact in any
    order (tests/test_hip_int8.py), with copies."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, dim), np.float32)
    for i in range(n):
        cols_ = np.concatenate([rs.choice(20, 12, replace=False), 20 + rs.choice(dim - 20, 4, replace=False)])
        rows[i, cols_] = rs.choice(np.array([0.25, -0.25], np.float32), 16)
    rows[1::8] = rows[0::8][: rows[1::8].shape[0]]
    return rows


def exact_index():
    """(stored rows, queries, an ExactIndex with a binary shadow) whose fp32 inner products are exact: the queries are rows
    times 2 (norm exactly 2), so the normalised query is the row and every partial sum a multiple of 1 / 16."""
    if "exact" not in _cache:
        n, dim = 3000, 128
        x = exact_dot_rows(n, dim, 3)
        idx = build_index(x, columns(n, 3), binary_shadow=True)
        stored = idx._corpus.emb.cpu().numpy()
        assert same_bits(stored, x), "rows of norm exactly 1 are stored as they are"
        q = (x[[0, 17, 33, 250, 1999, 2998]] * np.float32(2)).astype(np.float32)
        assert same_bits(im.normalize_query(q), x[[0, 17, 33, 250, 1999, 2998]])
        _cache["exact"] = (stored, q, idx)
    return _cache["exact"]


def model_search(idx, stored, q, k, eta, pref, cand, rescore):
    from dewi._engine import binary_cut
    corpus = idx._corpus
    c = binary_cut(k, cand, stored.shape[0])
    return bm.search(stored, host_bits(corpus.b1_bits), q, corpus.dewi32.cpu().numpy(), corpus.ent32.cpu().numpy(), k, eta, pref, c,
                     rescore=rescore)


@pytest.mark.parametrize("rescore", [True, False])
@pytest.mark.parametrize("eta,pref", [(0.0, 0.0), (0.3, 0.0), (0.3, 0.2)])
def test_search_equals_the_model_pipeline_bit_for_bit(eta, pref, rescore):
    stored, q, idx = exact_index()
    for k, cand in ((10, None), (7, 100), (5, 40), (60, None), (3, 1024)):
        rows, scores = idx.search_binary_batch(q, k, eta, pref, candidates=cand, rescore=rescore)
        want_ids, want_sc = model_search(idx, stored, q, k, eta, pref, cand, rescore)
        assert np.array_equal(rows, want_ids), (k, cand)
        assert same_bits(scores, want_sc), (k, cand)
    one = idx.search_binary(q[1], 5, eta, pref, rescore=rescore)
    want_ids, want_sc = model_search(idx, stored, q[1:2], 5, eta, pref, None, rescore)
    assert [int(r[0][1:]) for r in one] == want_ids[0].tolist()
    assert same_bits(np.array([r[1] for r in one], np.float32), want_sc[0])
    if not rescore and eta == 0.0:
        assert set(np.unique(scores * 128).tolist()) <= set(range(-128, 129)), "the blended Hamming sim is s / dim"


def gauss_index(dim, n=3000):
    if ("gauss", dim) not in _cache:
        x = np.random.RandomState(dim).randn(n, dim).astype(np.float32)
        q = np.random.RandomState(dim + 1).randn(6, dim).astype(np.float32)
        q[1] = x[49] + np.float32(0.3) * q[1]
        idx = build_index(x, columns(n, dim), cls="dewi", binary_shadow=True)
        _cache[("gauss", dim)] = (x, q, idx)
    return _cache[("gauss", dim)]


@pytest.mark.parametrize("dim", [128, 768])
def test_rescored_search_on_gaussian_rows_within_the_accumulation_bound(dim):
    from dewi._engine import binary_cut
    x, q, idx = gauss_index(dim)
    backend = idx._backend
    corpus = backend._corpus
    stored = corpus.emb.cpu().numpy()
    bound = dim * EPS * 1.0002
    qn = im.normalize_query(q).astype(np.float64)
    decisive = total = 0
    for k, cand in ((10, None), (100, None), (5, 64)):
        rows, scores = backend.search_binary_batch(q, k, 0.0, 0.0, candidates=cand)      # eta 0, pref 0: the score IS the fp32 sim
        c = binary_cut(k, cand, stored.shape[0])
        cut = bm.candidates(host_bits(corpus.b1_bits), bm.binarize(q), corpus.dewi32.cpu().numpy(), corpus.ent32.cpu().numpy(), c)["id"]
        for j in range(q.shape[0]):
            ref = stored[rows[j]].astype(np.float64) @ qn[j]
            err = np.abs(scores[j].astype(np.float64) - ref).max()
            print(f"dim {dim} k {k} cut {c} query {j}: max |score - float64| = {err:.3e} (bound {bound:.3e})")
            assert err <= bound
            assert set(rows[j].tolist()) <= set(cut[j].tolist())
            ref_cut = stored[cut[j]].astype(np.float64) @ qn[j]
            order = np.argsort(-ref_cut, kind="stable")
            top = ref_cut[order[: k + 1]]
            total += 1
            if np.min(top[:-1] - top[1:]) > 2 * bound:       # no two of the k + 1 best can change places in fp32
                decisive += 1
                assert rows[j].tolist() == cut[j][order[:k]].tolist(), (k, cand, j)
    assert decisive >= total // 3, (decisive, total)     # (the k = 100 cases rarely are: a hundred gaps)
    res = idx.search_binary(q[1], 10, 0.0, 0.0)
    assert res[0][0] == "d000049" and len(res) == 10
    batch = idx.search_binary_batch(q, 10, 0.0, 0.0)
    assert [r[0] for r in batch[1]] == [r[0] for r in res]


def test_cut_of_every_row_gives_the_exact_answer():
    x, q, idx = gauss_index(128)
    k = 10
    with pytest.raises(ValueError, match="at most 1024"):
        idx._backend.search_binary_batch(q, k, 0.0, 0.0, candidates=x.shape[0])
    small = build_index(x[:1000], columns(1000, 2), binary_shadow=True)
    sims = im.normalize_query(q).astype(np.float64) @ small._corpus.emb.cpu().numpy().astype(np.float64).T
    top = -np.sort(-sims, axis=1)[:, : k + 1]
    assert (top[:, k - 1] - top[:, k] > 1e-4).all(), "the inputs: no tie at the cut (fp32 sums err by 128 * 2^-24 = 7.6e-6)"
    for cand in (1000, 1024):
        rows, _ = small.search_binary_batch(q, k, 0.0, 0.0, candidates=cand)
        exact, _ = small.search_batch(q, k, 0.0, 0.0)
        for j in range(q.shape[0]):
            assert set(rows[j].tolist()) == set(exact[j].tolist()) == set(np.argsort(-sims[j])[:k].tolist()), (cand, j)


def test_mutated_index_equals_a_fresh_build():
    n, dim = 1500, 128
    x = np.random.RandomState(5).randn(n + 40, dim).astype(np.float32)
    cols = columns(n + 40, 5)
    ids = [f"d{i:06d}" for i in range(n + 40)]
    idx = build_index(x[:n], {k: v[:n] for k, v in cols.items()}, binary_shadow=True, int8_shadow=True)
    q = np.random.RandomState(6).randn(5, dim).astype(np.float32)
    idx.search_binary_batch(q, 10)                                         # the copy is in use before the mutation
    idx.remove([ids[i] for i in range(0, 300, 7)])
    assert idx._corpus._b1_stale and idx._corpus._i8_stale
    up = list(range(n, n + 40)) + [500, 501, 502]
    new_rows = x[up].copy()
    new_rows[-3:] = np.random.RandomState(7).randn(3, dim).astype(np.float32)
    idx.upsert_batch_columns([ids[i] for i in up], new_rows, {k: v[up] for k, v in cols.items()})
    assert idx._corpus._b1_stale
    raw = {ids[i]: x[i] for i in range(n + 40)}
    raw.update({ids[i]: r for i, r in zip(up, new_rows)})
    order = list(idx._doc_ids)
    pos = {d: i for i, d in enumerate(ids)}
    from dewi.backends import ExactIndex
    fresh = ExactIndex(dim, binary_shadow=True)
    fresh.add_batch_columns(order, np.stack([raw[d] for d in order]), {k: v[[pos[d] for d in order]] for k, v in cols.items()})
    fresh.build()
    for rescore in (False, True):
        a = idx.search_binary_batch(q, 10, 0.3, 0.2, rescore=rescore)
        b = fresh.search_binary_batch(q, 10, 0.3, 0.2, rescore=rescore)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    assert not idx._corpus._b1_stale
    assert np.array_equal(host_bits(idx._corpus.b1_bits), host_bits(fresh._corpus.b1_bits))
    assert np.array_equal(host_bits(idx._corpus.b1_bits), bm.binarize(idx._corpus.emb.cpu().numpy()))


def test_other_searches_are_unchanged_by_the_copy():
    n, dim = 3000, 128
    x = np.random.RandomState(dim).randn(n, dim).astype(np.float32)
    cols = columns(n, dim)
    q = np.random.RandomState(dim + 1).randn(6, dim).astype(np.float32)
    both = build_index(x, cols, binary_shadow=True, int8_shadow=True, batch_shadow=True)
    plain = build_index(x, cols, int8_shadow=True, batch_shadow=True)
    assert both._corpus.has_binary_shadow and not plain._corpus.has_binary_shadow
    for k in (10, 100):
        for kwargs in ({}, {"approx": True}, {"approx": False}, {"approx": True, "rescore": False}):
            a = both.search_batch(q, k, 0.3, 0.2, **kwargs)
            b = plain.search_batch(q, k, 0.3, 0.2, **kwargs)
            assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]), (k, kwargs)
            one_a = both.search(q[2], k, 0.3, 0.2, **kwargs)
            one_b = plain.search(q[2], k, 0.3, 0.2, **kwargs)
            assert [(r[0], r[1]) for r in one_a] == [(r[0], r[1]) for r in one_b]
    filt = np.arange(n) % 2 == 0
    a, b = both.search_batch(q, 5, 0.3, 0.0, filter=filt), plain.search_batch(q, 5, 0.3, 0.0, filter=filt)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])


def test_save_load_round_trip(tmp_path):
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    stored, q, idx = exact_index()
    idx.save(tmp_path / "ix")
    back = ExactIndex.load(tmp_path / "ix", binary_shadow=True)
    for rescore in (False, True):
        a = idx.search_binary_batch(q, 10, 0.3, 0.2, rescore=rescore)
        b = back.search_binary_batch(q, 10, 0.3, 0.2, rescore=rescore)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    assert np.array_equal(host_bits(back._corpus.b1_bits), host_bits(idx._corpus.b1_bits))
    plain = ExactIndex.load(tmp_path / "ix")
    with pytest.raises(ValueError, match="binary_shadow=True"):
        plain.search_binary_batch(q, 10)
    _, gq, gidx = gauss_index(128)
    gidx.save(tmp_path / "dx")
    gback = DewiIndex.load(tmp_path / "dx", binary_shadow=True)
    assert [[r[:2] for r in rs] for rs in gback.search_binary_batch(gq, 10)] == [[r[:2] for r in rs] for rs in gidx.search_binary_batch(gq, 10)]


def test_refusals():
    from dewi.backends import ExactIndex
    from dewi.ivf import IVFIndex
    stored, q, idx = exact_index()
    with pytest.raises(ValueError, match="binary_shadow"):
        IVFIndex(128, binary_shadow=True)
    plain = build_index(stored[:200], columns(200, 1))
    with pytest.raises(ValueError, match="binary_shadow=True"):
        plain.search_binary(q[0])
    with pytest.raises(ValueError, match="no binary shadow"):
        plain._corpus.search_binary(q, 5)
    with pytest.raises(ValueError, match="exceeds the cut"):
        idx.search_binary_batch(q, 30, candidates=20)
    with pytest.raises(ValueError, match="at most 1024"):
        idx.search_binary_batch(q, 10, candidates=2000)
    with pytest.raises(ValueError, match="Expected queries"):
        idx.search_binary_batch(q[:, :64], 10)
    with pytest.raises(ValueError, match="dim % 128"):
        ExactIndex(192, binary_shadow=True)

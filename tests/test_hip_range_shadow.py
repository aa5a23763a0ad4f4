"""GPU tests of the range search through the bf16 shadow (256 queries per corpus pass on the matrix cores, exact re-scoring)
and of the near-duplicate self-join built on it.

Contract: the shadow route returns what the dense route returns — the same lims and rows, similarities and adjusted scores
equal bit for bit — and the self-join reports the pair (a, b), a < b, iff row b is in range_search(E[a], threshold).

Inputs: the clustered generator of tests/test_hip_range.py (seed 0, noise 1.0) with 300 queries over N = 40 011 rows: a ragged
last tile, 1 251 tiles over the pass's workgroups (every workgroup cycles its three-slot ring), two groups of queries, the
second with 44 active.  Oracle tolerances are the project's (tests/parity.py): GAP = 5e-7 on a float64 similarity decides
whether a row is surely in or out, SCORE_TOL = 1e-5 on returned values, and parity.default_floor's 80 % of the queries must be
decisive.  Computed on the CPU with this generator in float64: 300 / 300 decisive at 0.6 and 297-300 / 300 at 0.3 for dims 256,
384 and 768 (1 to 692 rows per query at 0.3); at 0.0 about a quarter of the queries have a row inside the band, so that
threshold is used for bit-equality only.
"""
import functools

import numpy as np
import pytest

import dewi_oracle as orc
from parity import GAP, SCORE_TOL, default_floor

pytestmark = pytest.mark.gpu

N, NQ = 40011, 300
ETA = 0.4
DIMS = (256, 384, 768)
FIRST_ROW = 12345


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _clustered(n, d, seed, noise=1.0, n_queries=64, n_centres=64):
    r = np.random.RandomState(seed)
    cen = r.randn(n_centres, d)
    lab = r.randint(0, n_centres, n)
    X = _unit(cen[lab] + noise * r.randn(n, d))
    rows = r.choice(n, n_queries, replace=False)
    Q = _unit(X[rows] + 0.05 * r.randn(n_queries, d))
    return X, Q


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _mixed_thresholds():
    return np.array([(0.6, 0.3, 0.0)[j % 3] for j in range(NQ)], dtype=np.float32)


THRESHOLDS = {"0.6": 0.6, "0.3": 0.3, "0.0": 0.0, "mixed": None}


def _thr(name, nb=NQ):
    return _mixed_thresholds()[:nb] if name == "mixed" else THRESHOLDS[name]


class _Case:
    """One built index with a shadow and the dense route's answers, computed once and left unchanged."""

    def __init__(self, dim):
        import torch
        from dewi.backends import ExactIndex
        self.dim = dim
        self.X, self.Q = _clustered(N, dim, 0, noise=1.0, n_queries=NQ)
        self.cols = orc.synth_payload_columns(N, seed=0)
        self.index = ExactIndex(dim, "cosine", batch_shadow=True)
        self.index.add_batch_columns([f"doc_{i:07d}" for i in range(N)], self.X, self.cols)
        self.index.build()
        self.corpus = self.index._corpus
        assert self.corpus.shadow is not None
        with torch.cuda.device(self.corpus.device):
            self.q_dev = self.corpus.stage_queries(self.Q).clone()
        self._dense = {}

    def run(self, thr, pref, sort, nb=NQ, use_shadow=True, corpus=None, q_dev=None):
        import torch
        corpus = self.corpus if corpus is None else corpus
        q = self.q_dev if q_dev is None else q_dev
        with torch.cuda.device(corpus.device):
            out = corpus.range_search_routed(q[:nb], thr, ETA, pref, sort=sort, use_shadow=use_shadow)
            return tuple(t.cpu().numpy() for t in out)

    def dense(self, name, pref, sort):
        """The dense route's answer for all 300 queries (the reference of the bit-equality tests)."""
        key = (name, pref, sort)
        if key not in self._dense:
            self._dense[key] = self.run(_thr(name), pref, sort, use_shadow=False)
        return self._dense[key]

    def dense_prefix(self, name, pref, sort, nb):
        """... restricted to the first nb queries: every query's segment is its own, so it is a prefix."""
        lims, rows, sims, scores = self.dense(name, pref, sort)
        t = int(lims[nb])
        return lims[:nb + 1], rows[:t], sims[:t], scores[:t]


@functools.lru_cache(maxsize=None)
def _case(dim):
    return _Case(dim)


def _assert_same(got, want, what):
    lims, rows, sims, scores = got
    wl, wr, ws, wsc = want
    assert lims.dtype == np.int64 and rows.dtype == np.int64 and sims.dtype == np.float32 and scores.dtype == np.float32
    assert np.array_equal(lims, wl), f"{what}: lims differ (first at query {int(np.argmax(np.diff(lims) != np.diff(wl)))})"
    assert np.array_equal(rows, wr), f"{what}: rows differ"
    assert np.array_equal(_bits(sims), _bits(ws)), f"{what}: similarity bits differ"
    assert np.array_equal(_bits(scores), _bits(wsc)), f"{what}: score bits differ"


# ---------------------------------------------------------------------------------------------------- 1. bit-equality
@pytest.mark.parametrize("batch", [300, 256, 33, "range_shadow_min_batch"])
@pytest.mark.parametrize("dim", DIMS)
def test_shadow_route_is_bit_equal_to_the_dense_route(dim, batch):
    case = _case(dim)
    nb = int(case.corpus.range_shadow_min_batch) if batch == "range_shadow_min_batch" else batch
    assert 1 <= nb <= NQ
    for name in THRESHOLDS:
        for sort in (True, False):
            for pref in (0.0, 0.1):
                got = case.run(_thr(name, nb), pref, sort, nb=nb)
                _assert_same(got, case.dense_prefix(name, pref, sort, nb), f"dim {dim} batch {nb} thr {name} sort {sort} pref {pref}")
    # (the cases are not trivial: hundreds of rows per query at 0.3, and rows at 0.6 too)
    assert int(np.diff(case.dense("0.3", 0.0, True)[0]).max()) > 256 and int(case.dense("0.6", 0.0, True)[0][-1]) > 0


# ---------------------------------------------------------------------------------------------------- 2. the route is taken
def test_the_shadow_route_is_really_taken():
    import torch
    from dewi._engine import DeviceCorpus
    case = _case(256)
    c = case.corpus
    fresh = DeviceCorpus(c.emb, c.dewi32, c.ent32, "cosine").enable_bf16_shadow()
    assert fresh.shadow is not c.shadow
    fresh.shadow.zero_()
    torch.cuda.synchronize()
    lims, rows, sims, scores = case.run(0.3, 0.0, True, corpus=fresh)
    assert rows.size == 0 and not lims.any()                      # every shadow score is 0 < 0.3 - margin: nothing survives
    want = case.dense("0.3", 0.0, True)
    assert want[1].size > 0
    _assert_same(case.run(0.3, 0.0, True, corpus=fresh, use_shadow=False), want, "dense route next to a zeroed shadow")
    nb = int(fresh.range_shadow_min_batch) - 1                    # below the minimum: the dense answer, zeroed shadow or not
    assert nb >= 1
    _assert_same(case.run(0.3, 0.0, True, nb=nb, corpus=fresh), case.dense_prefix("0.3", 0.0, True, nb), "batch below the minimum")


# ---------------------------------------------------------------------------------------------------- 3. the oracle
def _in_search_order(rows, scores, sims):
    if rows.size < 2:
        return True
    a, b = scores[:-1], scores[1:]
    s, t = sims[:-1], sims[1:]
    return bool(np.all((a > b) | ((a == b) & ((s > t) | ((s == t) & (rows[:-1] < rows[1:]))))))


@pytest.mark.parametrize("dim", DIMS)
def test_shadow_route_vs_oracle(dim):
    case = _case(dim)
    E = case.index._embeddings
    dewi32, ent32 = orc.payload_soa(case.cols["dewi"], case.cols["ht_mean"], case.cols["hi_mean"])
    Qp = np.stack([orc.prepare_query(q, "cosine") for q in case.Q])
    s64 = Qp.astype(np.float64) @ E.astype(np.float64).T
    w_sim = abs(float(np.float32(1 - ETA)))
    for tau, pref in ((0.6, 0.0), (0.3, 0.1)):
        lims, rows, sims, scores = case.run(tau, pref, True)
        g = GAP * max(1.0, abs(tau))
        assert lims.shape == (NQ + 1,) and lims[0] == 0 and lims[-1] == rows.size == scores.size == sims.size
        decisive = 0
        for j in range(NQ):
            r = rows[lims[j]:lims[j + 1]]
            sc, sm = scores[lims[j]:lims[j + 1]], sims[lims[j]:lims[j + 1]]
            assert r.size == 0 or (r.min() >= 0 and r.max() < N), j
            assert np.unique(r).size == r.size, f"query {j}: duplicate rows"
            got = np.zeros(N, dtype=bool)
            got[r] = True
            sure_in = s64[j] >= tau + g
            sure_out = s64[j] < tau - g
            assert not np.any(sure_in & ~got), f"query {j}, tau {tau}: rows {np.nonzero(sure_in & ~got)[0][:5]} are missing"
            assert not np.any(sure_out & got), f"query {j}, tau {tau}: rows {np.nonzero(sure_out & got)[0][:5]} do not belong"
            decisive += int(not np.any(~sure_in & ~sure_out))
            if r.size:
                want_sim = (E[r] @ Qp[j]).astype(np.float32)               # the oracle's similarities() for these rows
                adj = (1 - ETA) * want_sim + ETA * dewi32[r]
                if pref != 0:
                    adj += pref * ent32[r]
                want_sc = adj.astype(np.float32)
                sim_tol = SCORE_TOL * max(1.0, float(np.abs(want_sim).max()))
                sc_tol = SCORE_TOL * max(1.0, float(np.abs(want_sc).max()), w_sim * max(1.0, abs(tau)))
                assert float(np.abs(sm.astype(np.float64) - want_sim).max()) <= sim_tol, f"query {j}, tau {tau}: similarity"
                assert float(np.abs(sc.astype(np.float64) - want_sc).max()) <= sc_tol, f"query {j}, tau {tau}: adjusted score"
            assert _in_search_order(r, sc, sm), f"query {j}, tau {tau}: not in search order"
        print(f"dim {dim} tau {tau}: {decisive}/{NQ} decisive, sizes {np.diff(lims).min()}..{np.diff(lims).max()}")
        assert decisive >= default_floor(10) * NQ, f"tau {tau}: only {decisive}/{NQ} decisive queries"


# ---------------------------------------------------------------------------------------------------- raw calls
def _raw(corpus, q_dev, thr, first_row=0, seg_cap=32, eta=ETA, pref=0.0):
    """dewi_knn_range_shadow_count + _collect as the library exports them: (counts with -1 for a flagged query, lims, rows,
    sims, scores in SEGMENT order)."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    nb = int(q_dev.shape[0])
    dev = corpus.device
    with torch.cuda.device(dev):
        t = corpus.stage_thresholds(thr, nb)
        need = int(lib.dewi_knn_range_shadow_workspace_bytes(corpus.n_rows, corpus.dim, 0, nb, seg_cap))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        counts_d = torch.empty(nb, dtype=torch.int64, device=dev)
        nat.check(lib.dewi_knn_range_shadow_count(nat.ptr(corpus.emb), nat.ptr(corpus.shadow), corpus.n_rows, corpus.dim, first_row,
                                                  nat.ptr(q_dev), nb, nat.ptr(t), seg_cap, nat.ptr(counts_d), nat.ptr(ws), need,
                                                  nat.stream_ptr()))
        counts = counts_d.cpu().numpy()
        lims = np.zeros(nb + 1, dtype=np.int64)
        np.cumsum(np.maximum(counts, 0), out=lims[1:])
        total = int(lims[-1])
        rows = torch.full((total + 8,), -7, dtype=torch.int64, device=dev)           # 8 guard elements behind the capacity
        sims = torch.full((total + 8,), -7.0, dtype=torch.float32, device=dev)
        scores = torch.full((total + 8,), -7.0, dtype=torch.float32, device=dev)
        nat.check(lib.dewi_knn_range_shadow_collect(nat.ptr(ws), need, corpus.n_rows, corpus.dim, first_row, nb, seg_cap,
                                                    nat.ptr(torch.from_numpy(lims).to(dev)), total, nat.ptr(corpus.dewi32),
                                                    nat.ptr(corpus.ent32), float(eta), float(pref), nat.ptr(rows), nat.ptr(sims),
                                                    nat.ptr(scores), nat.stream_ptr()))
        rows, sims, scores = rows.cpu().numpy(), sims.cpu().numpy(), scores.cpu().numpy()
    assert np.all(rows[total:] == -7) and np.all(sims[total:] == -7.0) and np.all(scores[total:] == -7.0)   # nothing at or beyond capacity
    return counts, lims, rows[:total], sims[:total], scores[:total]


def _ascending(lims, rows, sims, scores):
    """Every query's segment in ascending row order."""
    seg = np.repeat(np.arange(lims.size - 1), np.diff(lims))
    order = np.lexsort((rows, seg))
    return rows[order], sims[order], scores[order]


# ---------------------------------------------------------------------------------------------------- 4. overflow and repair
def test_overflowed_queries_are_flagged_and_repaired():
    case = _case(384)
    c = case.corpus
    counts, lims, rows, sims, scores = _raw(c, case.q_dev, 0.3, seg_cap=4)
    assert np.any(counts == -1) and np.any(counts >= 0), "seg_cap = 4 at 0.3 must flag some queries and answer others"
    want = case.dense("0.3", 0.0, False)
    ok = counts >= 0
    assert np.array_equal(counts[ok], np.diff(want[0])[ok])            # an answered query's count is the dense route's
    keep = np.repeat(ok, np.diff(want[0]))
    r, s, sc = _ascending(lims, rows, sims, scores)
    assert np.array_equal(r, want[1][keep]) and np.array_equal(_bits(s), _bits(want[2][keep]))
    assert np.array_equal(_bits(sc), _bits(want[3][keep]))
    try:                                                               # the Python route repairs the flagged ones
        c.range_shadow_seg_cap = 4
        for sort in (True, False):
            _assert_same(case.run(0.3, 0.0, sort), case.dense("0.3", 0.0, sort), f"seg_cap 4, sort {sort}")
    finally:
        c.range_shadow_seg_cap = 32


def test_every_row_passing_flags_every_query_and_the_answer_is_still_equal():
    case = _case(256)
    nb = 64                                                            # 64 x 40 011 rows: the property needs no more
    counts = _raw(case.corpus, case.q_dev[:nb], -1.0)[0]
    assert np.all(counts == -1)                     # ~40 rows per lane quarter of a workgroup, more than 32
    got = case.run(-1.0, 0.1, False, nb=nb)
    assert np.array_equal(np.diff(got[0]), np.full(nb, N))
    _assert_same(got, case.run(-1.0, 0.1, False, nb=nb, use_shadow=False), "threshold -1")


# ---------------------------------------------------------------------------------------------------- 5. first_row
def test_first_row_restricts_the_scan():
    case = _case(768)
    c = case.corpus
    for pref in (0.0, 0.1):
        c0, l0, r0, s0, sc0 = _raw(c, case.q_dev, 0.3, first_row=0, pref=pref)
        c1, l1, r1, s1, sc1 = _raw(c, case.q_dev, 0.3, first_row=FIRST_ROW, pref=pref)
        assert np.all(c0 >= 0) and np.all(c1 >= 0)
        assert r1.size > 0 and r1.min() >= FIRST_ROW and r0.min() < FIRST_ROW
        r0, s0, sc0 = _ascending(l0, r0, s0, sc0)
        r1, s1, sc1 = _ascending(l1, r1, s1, sc1)
        keep = r0 >= FIRST_ROW
        seg = np.repeat(np.arange(NQ), np.diff(l0))
        assert np.array_equal(np.bincount(seg[keep], minlength=NQ), c1)
        assert np.array_equal(r0[keep], r1) and np.array_equal(_bits(s0[keep]), _bits(s1))
        assert np.array_equal(_bits(sc0[keep]), _bits(sc1))


# ---------------------------------------------------------------------------------------------------- 6. edges
def test_edges():
    import torch
    case = _case(256)
    c = case.corpus
    # a duplicated query gives two identical segments
    q = case.q_dev.clone()
    q[1] = q[0]
    q[NQ - 1] = q[0]
    for sort in (True, False):
        lims, rows, sims, scores = case.run(0.3, 0.1, sort, q_dev=q)
        assert lims[1] - lims[0] > 0
        for j in (1, NQ - 1):
            assert lims[j + 1] - lims[j] == lims[1] - lims[0]
            assert np.array_equal(rows[lims[j]:lims[j + 1]], rows[:lims[1]])
            assert np.array_equal(_bits(sims[lims[j]:lims[j + 1]]), _bits(sims[:lims[1]]))
            assert np.array_equal(_bits(scores[lims[j]:lims[j + 1]]), _bits(scores[:lims[1]]))
    # an all-zero query: similarity 0 to every row
    q = case.q_dev[:64].clone()
    q[5] = 0.0
    for tau in (-0.5, 0.5):
        got = case.run(tau, 0.0, True, nb=64, q_dev=q)
        _assert_same(got, case.run(tau, 0.0, True, nb=64, q_dev=q, use_shadow=False), f"zero query, threshold {tau}")
        assert got[0][6] - got[0][5] == (N if tau < 0 else 0)
    # a threshold nothing reaches
    lims, rows, sims, scores = case.run(1.5, 0.0, True)
    assert not lims.any() and lims.shape == (NQ + 1,) and rows.size == sims.size == scores.size == 0
    # max_results raises before the collect
    total = int(case.dense("0.3", 0.0, True)[0][-1])
    with torch.cuda.device(c.device):
        with pytest.raises(ValueError, match="max_results"):
            c.range_search_device(case.q_dev, 0.3, ETA, 0.0, max_results=total - 1)
        assert int(c.range_search_device(case.q_dev, 0.3, ETA, 0.0, max_results=total)[0][-1]) == total
    # two runs write identical bytes (segment order from the raw calls, ascending rows from the Python route)
    a, b = _raw(c, case.q_dev, 0.3), _raw(c, case.q_dev, 0.3)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    a, b = case.run(0.3, 0.0, False), case.run(0.3, 0.0, False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_a_seg_cap_beyond_the_32_bit_offsets_is_refused():
    from dewi import _native as nat
    lib = nat.load_library()
    case = _case(256)
    c = case.corpus
    # 4 x 256 workgroups x 256 queries x 8 bytes = 2 MiB per record of seg_cap on a 256-CU device: 2048 records = 2^32 bytes
    cus = nat.ctypes.c_int(0)
    nat.check(lib.dewi_device_info(nat.ctypes.byref(cus), None, None))
    blocks = min(cus.value, (N + 31) // 32)
    too_many = (1 << 32) // (4 * blocks * 256 * 8) + 1
    assert lib.dewi_knn_range_shadow_workspace_bytes(N, 256, 0, NQ, too_many) == 0
    assert lib.dewi_knn_range_shadow_workspace_bytes(N, 256, 0, NQ, 32) > 0
    p = nat.ptr(c.emb)
    rc = lib.dewi_knn_range_shadow_count(p, nat.ptr(c.shadow), N, 256, 0, nat.ptr(case.q_dev), NQ, nat.ptr(case.q_dev), too_many,
                                         nat.ptr(case.q_dev), p, 1 << 40, None)
    assert rc == nat.ERR_INVALID_ARG


# ---------------------------------------------------------------------------------------------------- 7. near_duplicates
ND_N = 12011


class _DupCase:
    """N = 12 011 clustered rows with planted near-copies: 200 rows overwritten by slightly perturbed other rows, 40 exact
    copies of one row scattered through the corpus, 8 exact copies in a row."""

    def __init__(self, dim, n=ND_N, space="cosine", shadow=True):
        from dewi.backends import ExactIndex
        self.dim, self.n = dim, n
        X, _ = _clustered(n, dim, 0, noise=1.0, n_queries=NQ)
        r = np.random.RandomState(1)
        run0 = n // 3
        free = np.setdiff1d(np.arange(n), np.arange(run0, run0 + 8))
        perm = r.permutation(free)
        dst, src = perm[:200], perm[200:400]
        X[dst] = _unit(X[src] + 0.01 * r.randn(200, dim))
        X[perm[400:440]] = X[perm[440]]
        X[run0:run0 + 8] = X[perm[441]]
        self.X = X
        self.ids = [f"doc_{i:07d}" for i in range(n)]
        self.index = ExactIndex(dim, space, batch_shadow=shadow)
        self.index.add_batch_columns(self.ids, X, orc.synth_payload_columns(n, seed=0))
        self.index.build()
        self.corpus = self.index._corpus

    def oracle_pairs(self, tau, space="cosine"):
        """{(a, b): a < b, s64 >= tau} with the float64 similarity of prepared query a against stored row b, and the
        smallest distance of any similarity from tau."""
        E = self.index._embeddings
        E64 = E.astype(np.float64)
        e2 = (E64 * E64).sum(1)
        aa, bb, margin = [], [], np.inf
        for lo in range(0, self.n, 1024):                       # blocks of query rows: the full matrix is 1.2 GB
            hi = min(self.n, lo + 1024)
            Qp = np.stack([orc.prepare_query(e, space) for e in E[lo:hi]]).astype(np.float64)
            S = Qp @ E64.T
            if space == "l2":       # -||e - q||^2 expanded: in float64 the cancellation costs ~1e-15, far below GAP
                S = -(e2[None, :] + (Qp * Qp).sum(1)[:, None] - 2.0 * S)
            upper = np.arange(self.n)[None, :] > np.arange(lo, hi)[:, None]
            a, b = np.nonzero(upper & (S >= tau))
            aa.append(a + lo)
            bb.append(b)
            margin = min(margin, float(np.abs(S - tau)[upper].min()) if upper.any() else np.inf)
        return np.concatenate(aa), np.concatenate(bb), margin


@functools.lru_cache(maxsize=None)
def _dup_case(dim):
    return _DupCase(dim)


def _nd(corpus, *args, **kw):
    import torch
    with torch.cuda.device(corpus.device):
        return tuple(t.cpu().numpy() for t in corpus.near_duplicates_device(*args, **kw))


@pytest.mark.parametrize("dim", [256, 384])
def test_near_duplicates_finds_exactly_the_planted_pairs(dim):
    case = _dup_case(dim)
    assert case.corpus.shadow is not None
    a64, b64, margin = case.oracle_pairs(0.9)
    assert margin > GAP, f"an oracle similarity lies within {margin:.2e} of the threshold"
    assert a64.size >= 200 + 40 * 39 // 2 + 8 * 7 // 2
    a, b, sims = case.index.near_duplicates(0.9)
    assert a.dtype == np.int64 and b.dtype == np.int64 and sims.dtype == np.float32
    assert np.array_equal(a, a64) and np.array_equal(b, b64)                 # ordered by (a, b), as np.nonzero is
    assert np.all(sims >= np.float32(0.9))
    # (e) doc ids
    ia, ib, s2 = case.index.near_duplicates(0.9, doc_ids=True)
    assert ia == [case.ids[i] for i in a] and ib == [case.ids[i] for i in b] and np.array_equal(_bits(s2), _bits(sims))
    # (d) max_pairs
    with pytest.raises(ValueError, match="max_pairs"):
        case.index.near_duplicates(0.9, max_pairs=a.size - 1)
    assert case.index.near_duplicates(0.9, max_pairs=a.size)[0].size == a.size
    with pytest.raises(ValueError, match="max_pairs"):
        _nd(case.corpus, 0.5, max_pairs=1000)


@pytest.mark.parametrize("dim", [256, 384])
def test_near_duplicates_equal_the_dense_range_search_of_every_row(dim):
    import torch
    case = _dup_case(dim)
    c = case.corpus
    with torch.cuda.device(c.device):
        lims, rows, sims, _ = (t.cpu().numpy() for t in c.range_search_routed(c.emb, 0.5, 0.0, 0.0, sort=False, use_shadow=False))
    hits = np.diff(lims)
    assert hits.max() > 100 and hits.min() >= 1          # every row finds itself, and up to its whole cluster
    qa = np.repeat(np.arange(case.n), hits)
    keep = rows > qa
    want = (qa[keep], rows[keep], sims[keep])
    for kw in ({}, {"chunk": 256}, {"chunk": 2048}, {"use_shadow": False}):
        a, b, s = _nd(c, 0.5, **kw)
        assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]), kw
        assert np.array_equal(_bits(s), _bits(want[2])), kw


@pytest.mark.parametrize("space,shadow,tau", [("cosine", False, 0.9), ("l2", True, -0.2), ("l2", False, -0.2)])
def test_near_duplicates_without_a_shadow_route(space, shadow, tau):
    case = _DupCase(256, n=3000, space=space, shadow=shadow)
    assert case.corpus.shadow is None                                        # (an l2 index keeps no shadow)
    a64, b64, margin = case.oracle_pairs(tau, space)
    assert margin > GAP * max(1.0, abs(tau)) and a64.size >= 200
    a, b, sims = case.index.near_duplicates(tau)
    assert np.array_equal(a, a64) and np.array_equal(b, b64)
    assert np.all(sims >= np.float32(tau))

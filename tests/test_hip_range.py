"""GPU tests of the range search: every row whose similarity to the query is at least a threshold.

Contract: steps 1-2 of the reference's ExactIndex.search (src/dewi/backends.py:420-436) for every scanned row, the test
``sim >= threshold`` instead of the cut, then the blend of :461-465 — a row's similarity and adjusted score are bit for bit
what the one-query search gives it.  Inputs: the clustered corpus of tests/test_hip_ivf.py (20000 rows, 64 queries, seed 0).

Tolerances are the project's (tests/parity.py): GAP = 5e-7 on a float64 similarity decides whether a row is surely in or
surely out (scaled by max(1, |threshold|)), SCORE_TOL = 1e-5 on returned values (scaled as parity.compare_query scales it).
A (query, threshold) pair is decisive when no row lies inside the band; every case needs parity.default_floor's 80 %.
"""
import functools

import numpy as np
import pytest

import dewi_oracle as orc
from parity import GAP, SCORE_TOL, default_floor

pytestmark = pytest.mark.gpu

N, NQ = 20000, 64
ETA = 0.4
THRESHOLDS = {"cosine": (0.9, 0.6, 0.3), "l2": (-0.2, -0.8, -1.4)}
HALF = {"cosine": 0.0, "l2": -2.0}          # about half the corpus per query


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


class _Case:
    """One built index and the oracle's view of it, computed once and left unchanged."""

    def __init__(self, dim, space):
        from dewi.backends import ExactIndex
        self.dim, self.space = dim, space
        self.X, self.Q = _clustered(N, dim, 0)
        self.cols = orc.synth_payload_columns(N, seed=0)
        self.ids = [f"doc_{i:07d}" for i in range(N)]
        self.index = ExactIndex(dim, space)
        self.index.add_batch_columns(self.ids, self.X, self.cols)
        self.index.build()
        self.E = self.index._embeddings
        self.dewi32, self.ent32 = orc.payload_soa(self.cols["dewi"], self.cols["ht_mean"], self.cols["hi_mean"])
        self.Qp = np.stack([orc.prepare_query(q, space) for q in self.Q])
        self.s32 = np.stack([orc.similarities(self.E, qp, space) for qp in self.Qp])
        E64, Q64 = self.E.astype(np.float64), self.Qp.astype(np.float64)
        if space == "l2":       # -||e - q||^2 expanded: in float64 the cancellation costs ~1e-15, far below GAP
            self.s64 = -((E64 * E64).sum(1)[None, :] + (Q64 * Q64).sum(1)[:, None] - 2.0 * (Q64 @ E64.T))
        else:
            self.s64 = Q64 @ E64.T

    def blend32(self, j, rows, eta, pref):
        """The oracle's fp32 blend (backends.py:461-465) of query j for given rows."""
        adj = (1 - eta) * self.s32[j, rows] + eta * self.dewi32[rows]
        if pref != 0:
            adj += pref * self.ent32[rows]
        return adj.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(dim, space):
    return _Case(dim, space)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _in_search_order(rows, scores, sims):
    """Adjusted score descending, ties to the higher similarity, then to the lower row."""
    if rows.size < 2:
        return True
    a, b = scores[:-1], scores[1:]
    s, t = sims[:-1], sims[1:]
    ok = (a > b) | ((a == b) & ((s > t) | ((s == t) & (rows[:-1] < rows[1:]))))
    return bool(np.all(ok))


def _check_against_oracle(case, tau, eta, pref, lims, rows, scores, sims):
    """Every query of one call against the float64 similarities; returns the number of decisive queries."""
    g = GAP * max(1.0, abs(tau))
    assert lims.shape == (NQ + 1,) and lims[0] == 0 and lims[-1] == rows.size == scores.size == sims.size
    w_sim = abs(float(np.float32(1 - eta)))
    decisive = 0
    for j in range(NQ):
        r = rows[lims[j]:lims[j + 1]]
        sc, sm = scores[lims[j]:lims[j + 1]], sims[lims[j]:lims[j + 1]]
        s64 = case.s64[j]
        assert r.size == 0 or (r.min() >= 0 and r.max() < N), j
        assert np.unique(r).size == r.size, f"query {j}: duplicate rows"
        got = np.zeros(N, dtype=bool)
        got[r] = True
        sure_in = s64 >= tau + g
        sure_out = s64 < tau - g
        assert not np.any(sure_in & ~got), f"query {j}, tau {tau}: rows {np.nonzero(sure_in & ~got)[0][:5]} are missing"
        assert not np.any(sure_out & got), f"query {j}, tau {tau}: rows {np.nonzero(sure_out & got)[0][:5]} do not belong"
        decisive += int(not np.any(~sure_in & ~sure_out))
        if r.size:
            want_sim = case.s32[j, r]
            want_sc = case.blend32(j, r, eta, pref)
            sim_tol = SCORE_TOL * max(1.0, float(np.abs(want_sim).max()))
            sc_tol = SCORE_TOL * max(1.0, float(np.abs(want_sc).max()), w_sim * max(1.0, abs(tau)))
            err_sim = float(np.abs(sm.astype(np.float64) - want_sim.astype(np.float64)).max())
            err_sc = float(np.abs(sc.astype(np.float64) - want_sc.astype(np.float64)).max())
            assert err_sim <= sim_tol, f"query {j}, tau {tau}: similarity off by {err_sim:.3e} > {sim_tol:.1e}"
            assert err_sc <= sc_tol, f"query {j}, tau {tau}: adjusted score off by {err_sc:.3e} > {sc_tol:.1e}"
        assert _in_search_order(r, sc, sm), f"query {j}, tau {tau}: not in search order"
    return decisive


# ---------------------------------------------------------------------------------------------------- a. the oracle
@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [64, 96, 50, 129, 768])
def test_range_vs_oracle(dim, space):
    case = _case(dim, space)
    sizes = []
    for i, tau in enumerate(THRESHOLDS[space]):
        pref = 0.1 if i == 1 else 0.0
        lims, rows, scores, sims = case.index.range_search_batch(case.Q, tau, ETA, pref)
        dec = _check_against_oracle(case, tau, ETA, pref, lims, rows, scores, sims)
        print(f"dim {dim} {space} tau {tau}: {dec}/{NQ} decisive, sizes {np.diff(lims).min()}..{np.diff(lims).max()}")
        assert dec >= default_floor(10) * NQ, f"tau {tau}: only {dec}/{NQ} decisive queries"
        sizes.append(np.diff(lims))
    assert max(int(s.max()) for s in sizes) > 256 and min(int(s.min()) for s in sizes) <= 1


@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [64, 96, 50, 129])
def test_range_half_the_corpus_vs_oracle(dim, space):
    case = _case(dim, space)
    tau = HALF[space]
    lims, rows, scores, sims = case.index.range_search_batch(case.Q, tau, ETA, 0.0)
    dec = _check_against_oracle(case, tau, ETA, 0.0, lims, rows, scores, sims)
    print(f"dim {dim} {space} tau {tau}: {dec}/{NQ} decisive, sizes {np.diff(lims).min()}..{np.diff(lims).max()}")
    assert dec >= default_floor(10) * NQ, f"only {dec}/{NQ} decisive queries"
    assert int(np.diff(lims).max()) > N // 4


# ---------------------------------------------------------------------------------------------------- b. the search itself
def _equals_the_search(search, Q, lims, rows, scores, queries):
    """Query j's sorted range result == the search with k = candidates = its count: ids equal, scores bit-equal."""
    compared = 0
    for j in queries:
        m = int(lims[j + 1] - lims[j])
        if m == 0:
            continue
        ids, sc = search(Q[j:j + 1], m)
        assert np.array_equal(ids[0], rows[lims[j]:lims[j + 1]]), f"query {j} (m = {m}): ids differ"
        assert np.array_equal(_bits(sc[0]), _bits(scores[lims[j]:lims[j + 1]])), f"query {j} (m = {m}): scores differ"
        compared += 1
    return compared


@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [64, 96, 50, 129, 768])
def test_range_is_bit_equal_to_the_search(dim, space):
    case = _case(dim, space)
    idx = case.index
    for pref in (0.0, 0.1):
        search = lambda q, m: idx.search_batch(q, m, ETA, pref, candidates=m)             # noqa: E731
        lims, rows, scores, _ = idx.range_search_batch(case.Q, THRESHOLDS[space][1], ETA, pref)
        assert _equals_the_search(search, case.Q, lims, rows, scores, range(NQ)) >= 8
        # the widest threshold: counts beyond what the search keeps in per-wave lists (256)
        lims, rows, scores, _ = idx.range_search_batch(case.Q[:16], THRESHOLDS[space][2], ETA, pref)
        assert int(np.diff(lims).max()) > 256
        assert _equals_the_search(search, case.Q, lims, rows, scores, range(16)) == 16
    if dim != 768:              # about half the corpus: beyond what the search sorts in LDS (2048)
        lims, rows, scores, _ = idx.range_search_batch(case.Q[:2], HALF[space], ETA, 0.1)
        assert int(np.diff(lims).min()) > 2048
        assert _equals_the_search(lambda q, m: idx.search_batch(q, m, ETA, 0.1, candidates=m), case.Q, lims, rows, scores, range(2)) == 2


@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_range_is_bit_equal_to_the_search_bf16(space):
    import torch
    case = _case(96, space)
    cb = case.index._corpus.to_bf16()
    for pref in (0.0, 0.1):
        with torch.cuda.device(cb.device):
            out = cb.range_search_device(cb.stage_queries(case.Q), THRESHOLDS[space][1], ETA, pref)
            lims, rows, sims, scores = (t.cpu().numpy() for t in out)
        search = lambda q, m: cb.search(q, m, ETA, pref, candidates=m)                    # noqa: E731
        assert _equals_the_search(search, case.Q, lims, rows, scores, range(NQ)) >= 8
    with pytest.raises(NotImplementedError):
        cb.range_search_device(cb.stage_queries(case.Q[:1]), 0.5, ETA, 0.0, filter=cb.make_filter(np.ones(N, dtype=bool)))


@pytest.mark.parametrize("dim,space", [(64, "cosine"), (50, "cosine"), (129, "l2"), (768, "l2")])
def test_filtered_range_is_bit_equal_to_the_filtered_search(dim, space):
    case = _case(dim, space)
    idx = case.index
    mask = np.random.RandomState(dim).rand(N) < 0.5
    flt = idx.make_filter(mask)
    for pref in (0.0, 0.1):
        search = lambda q, m: idx.search_batch(q, m, ETA, pref, candidates=m, filter=flt)  # noqa: E731
        lims, rows, scores, _ = idx.range_search_batch(case.Q, THRESHOLDS[space][1], ETA, pref, filter=flt)
        assert mask[rows].all()
        assert _equals_the_search(search, case.Q, lims, rows, scores, range(NQ)) >= 8
    # the unprepared forms of the same list, and exactly the allowed rows of the unfiltered answer
    full = idx.range_search_batch(case.Q[:5], THRESHOLDS[space][1], ETA, 0.1, sort=False)
    want = idx.range_search_batch(case.Q[:5], THRESHOLDS[space][1], ETA, 0.1, filter=flt, sort=False)
    for f in (mask, np.nonzero(mask)[0], [case.ids[r] for r in np.nonzero(mask)[0]]):
        got = idx.range_search_batch(case.Q[:5], THRESHOLDS[space][1], ETA, 0.1, filter=f, sort=False)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
    for j in range(5):
        r = full[1][full[0][j]:full[0][j + 1]]
        keep = mask[r]
        assert np.array_equal(r[keep], want[1][want[0][j]:want[0][j + 1]])                 # ascending rows, bucketed filters too
        assert np.array_equal(_bits(full[2][full[0][j]:full[0][j + 1]][keep]), _bits(want[2][want[0][j]:want[0][j + 1]]))


# ---------------------------------------------------------------------------------------------------- c. batches, thresholds
@pytest.mark.parametrize("dim,space", [(64, "cosine"), (768, "cosine"), (129, "l2"), (50, "l2")])
def test_batches_equal_single_queries(dim, space):
    case = _case(dim, space)
    idx = case.index
    Q70 = np.concatenate([case.Q, case.X[:6]])                     # 70 queries: three chunks (32, 32, 6) of multi-query passes
    taus = THRESHOLDS[space]
    per_query = np.array([taus[j % 3] for j in range(70)], dtype=np.float32)
    for thr in (taus[1], per_query):
        lims, rows, scores, sims = idx.range_search_batch(Q70, thr, ETA, 0.1)
        assert lims.shape == (71,) and lims[-1] == rows.size
        for j in range(70):
            t = float(thr if np.isscalar(thr) else thr[j])
            l1, r1, sc1, sm1 = idx.range_search_batch(Q70[j:j + 1], t, ETA, 0.1)
            assert l1.tolist() == [0, lims[j + 1] - lims[j]], j
            assert np.array_equal(r1, rows[lims[j]:lims[j + 1]]), j
            assert np.array_equal(_bits(sc1), _bits(scores[lims[j]:lims[j + 1]])), j
            assert np.array_equal(_bits(sm1), _bits(sims[lims[j]:lims[j + 1]])), j
    # unsorted: strictly ascending rows holding the same (row, score, similarity) triples
    lims_u, rows_u, scores_u, sims_u = idx.range_search_batch(Q70, per_query, ETA, 0.1, sort=False)
    assert np.array_equal(lims_u, lims)
    for j in range(70):
        a, b = slice(lims[j], lims[j + 1]), np.argsort(rows[lims[j]:lims[j + 1]], kind="stable")
        assert np.all(np.diff(rows_u[a]) > 0), j
        assert np.array_equal(rows_u[a], rows[a][b]) and np.array_equal(_bits(scores_u[a]), _bits(scores[a][b]))
        assert np.array_equal(_bits(sims_u[a]), _bits(sims[a][b]))
    # the same call twice: the same bytes
    again = idx.range_search_batch(Q70, per_query, ETA, 0.1, sort=False)
    for x, y in zip(again, (lims_u, rows_u, scores_u, sims_u)):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------- d. edges
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_thresholds_beyond_every_score(space):
    case = _case(64, space)
    idx = case.index
    lims, rows, scores, sims = idx.range_search_batch(case.Q[:3], 2.0 if space == "cosine" else 1e-3, ETA)
    assert lims.tolist() == [0, 0, 0, 0] and rows.size == scores.size == sims.size == 0
    assert idx.range_search(case.Q[0], 2.0 if space == "cosine" else 1e-3) == []
    lims, rows, scores, sims = idx.range_search_batch(case.Q[:3], -2.0 if space == "cosine" else -5.0, ETA, sort=False)
    assert lims.tolist() == [0, N, 2 * N, 3 * N]
    assert np.array_equal(rows, np.tile(np.arange(N), 3))
    for j in range(3):
        assert np.abs(sims[j * N:(j + 1) * N].astype(np.float64) - case.s32[j]).max() <= SCORE_TOL * max(1.0, np.abs(case.s32[j]).max())
    with pytest.raises(ValueError, match="max_results"):
        idx.range_search_batch(case.Q[:3], -5.0, ETA, max_results=3 * N - 1)
    assert idx.range_search_batch(case.Q[:3], -5.0, ETA, max_results=3 * N)[0][-1] == 3 * N
    with pytest.raises(ValueError, match="max_results"):
        idx.range_search(case.Q[0], -5.0, max_results=10)


def test_a_row_equal_to_the_threshold_passes_and_nan_rows_never_do():
    from dewi.backends import ExactIndex
    n, dim = 3000, 96
    X, Q = _clustered(n, dim, 1, n_queries=4)
    X[7] = 0.0                                                     # a zero-norm row: stored as NaN (reference backends.py:403-405)
    X[2999] = 0.0
    cols = orc.synth_payload_columns(n, seed=1)
    idx = ExactIndex(dim, "cosine")
    idx.add_batch_columns([f"d{i}" for i in range(n)], X, cols)
    idx.build()
    assert np.isnan(idx._embeddings[7]).all()
    for thr in (-2.0, float("-inf")):
        lims, rows, scores, sims = idx.range_search_batch(Q, thr, ETA, sort=False)
        assert np.diff(lims).tolist() == [n - 2] * 4
        assert 7 not in rows and 2999 not in rows and not np.isnan(sims).any()
    assert idx.range_search_batch(Q, float("nan"), ETA)[0].tolist() == [0] * 5
    # the threshold set to a row's own similarity: that row passes, and so does exactly every row at or above it
    lims, rows, _, sims = idx.range_search_batch(Q[:1], 0.5, ETA, sort=False)
    assert lims[1] >= 2
    tau = float(np.sort(sims)[sims.size // 2])
    l2, r2, _, s2 = idx.range_search_batch(Q[:1], tau, ETA, sort=False)
    assert np.array_equal(r2, rows[sims >= np.float32(tau)]) and s2.min() == np.float32(tau)


def test_empty_and_tiny_filters():
    case = _case(64, "cosine")
    idx = case.index
    lims, rows, scores, sims = idx.range_search_batch(case.Q[:4], -2.0, ETA, filter=np.zeros(N, dtype=bool))
    assert lims.tolist() == [0] * 5 and rows.size == 0
    assert idx.range_search(case.Q[0], -2.0, filter=np.zeros(N, dtype=bool)) == []
    lims, rows, scores, sims = idx.range_search_batch(case.Q[:4], -2.0, ETA, filter=[5, 19999, 4097], sort=False)
    assert np.diff(lims).tolist() == [3] * 4 and rows.tolist() == [5, 4097, 19999] * 4
    other = _case(96, "cosine").index.make_filter(np.ones(N, dtype=bool))
    with pytest.raises(ValueError, match="another corpus"):
        idx.range_search_batch(case.Q[:1], 0.5, ETA, filter=other)


def test_the_facade_returns_doc_ids_and_payloads():
    from dewi.index import DewiIndex
    case = _case(64, "cosine")
    face = DewiIndex(64, rerank_eta=ETA, entropy_pref=0.1)
    face.add_batch_columns(case.ids, case.X, case.cols)
    res = face.range_search(case.Q[0], 0.6)                        # builds on first use, constructor defaults
    lims, rows, scores, _ = case.index.range_search_batch(case.Q[:1], 0.6, ETA, 0.1)
    assert len(res) == lims[1] >= 1
    assert [r[0] for r in res] == [case.ids[i] for i in rows]
    assert np.array_equal(_bits(np.array([r[1] for r in res], np.float32)), _bits(scores))
    for (doc, _, payload), row in zip(res[:5], rows[:5]):
        assert payload.dewi == pytest.approx(case.cols["dewi"][row])
        assert face.get_payload(doc).dewi == payload.dewi
    both = face.range_search_batch(case.Q[:2], [0.6, 2.0], eta=0.0, entropy_pref=0.0)
    assert len(both) == 2 and both[1] == [] and len(both[0]) == len(res)
    assert all(a[1] >= b[1] for a, b in zip(both[0][:-1], both[0][1:]))
    one = case.index.range_search(case.Q[0], 0.6, ETA, 0.1)
    assert [(r[0], np.float32(r[1]).view(np.uint32)) for r in one] == [(r[0], np.float32(r[1]).view(np.uint32)) for r in res]


def test_ivf_index_range_search_is_the_exact_one():
    from dewi.ivf import IVFIndex
    case = _case(64, "cosine")
    ivf = IVFIndex(64, "cosine", nlist=64, nprobe=1, train_iters=2)
    ivf.add_batch_columns(case.ids, case.X, case.cols)
    got = ivf.range_search_batch(case.Q[:9], 0.6, ETA, 0.1)
    want = case.index.range_search_batch(case.Q[:9], 0.6, ETA, 0.1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and got[0][-1] > 0


# ---------------------------------------------------------------------------------------------------- e. the C ABI itself
@pytest.mark.parametrize("n", [3001, 1025, 63])
def test_odd_row_counts(n):
    """An odd number of scanned rows puts every second query's keys on an odd 8-byte index (the selection loads aligned
    pairs), 1025 rows one key into a second chunk: the batch equals the single queries, which equal the float64 band."""
    from dewi.backends import ExactIndex
    dim = 96
    X, Q = _clustered(n, dim, 3, n_queries=7)
    cols = orc.synth_payload_columns(n, seed=3)
    idx = ExactIndex(dim, "cosine")
    idx.add_batch_columns([f"d{i}" for i in range(n)], X, cols)
    idx.build()
    E64 = idx._embeddings.astype(np.float64)
    for tau in (0.3, -2.0):
        lims, rows, scores, sims = idx.range_search_batch(Q, tau, ETA, 0.1, sort=False)
        for j in range(7):
            one = idx.range_search_batch(Q[j:j + 1], tau, ETA, 0.1, sort=False)
            seg = slice(lims[j], lims[j + 1])
            assert np.array_equal(one[1], rows[seg]) and np.array_equal(_bits(one[2]), _bits(scores[seg]))
            assert np.array_equal(_bits(one[3]), _bits(sims[seg]))
            s64 = E64 @ orc.prepare_query(Q[j], "cosine").astype(np.float64)
            got = np.zeros(n, dtype=bool)
            got[rows[seg]] = True
            assert not np.any((s64 >= tau + GAP * max(1.0, abs(tau))) & ~got) and not np.any((s64 < tau - GAP * max(1.0, abs(tau))) & got)
    assert lims[-1] == 7 * n                                       # (tau = -2: every row of every query)


def test_collect_never_writes_beyond_capacity_or_lims():
    import torch
    from dewi import _native as nat
    case = _case(64, "cosine")
    corpus = case.index._corpus
    lib, dev, nq = corpus._lib, corpus.device, 5
    q = torch.from_numpy(case.Q[:nq]).to(dev)
    thr = torch.full((nq,), 0.3, dtype=torch.float32, device=dev)
    need = lib.dewi_knn_range_workspace_bytes(N, 64, 0, nq)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.empty(nq, dtype=torch.int64, device=dev)
    nat.check(lib.dewi_knn_range_count(nat.ptr(corpus.emb), 0, N, 64, None, 0, nat.ptr(q), nq, nat.ptr(thr), 0, nat.ptr(counts),
                                       nat.ptr(ws), need, nat.stream_ptr()))
    c = counts.cpu().numpy()
    full = np.concatenate([[0], np.cumsum(c)])
    total = int(full[-1])
    assert c.min() > 8
    want = case.index.range_search_batch(case.Q[:nq], 0.3, ETA, 0.0, sort=False)

    def collect(lims_h, capacity):
        lims = torch.from_numpy(np.asarray(lims_h, dtype=np.int64)).to(dev)
        rows = torch.full((total + 16,), -7, dtype=torch.int64, device=dev)
        sims = torch.full((total + 16,), -7.0, dtype=torch.float32, device=dev)
        scores = torch.full((total + 16,), -7.0, dtype=torch.float32, device=dev)
        nat.check(lib.dewi_knn_range_collect(nat.ptr(ws), need, N, nq, nat.ptr(thr), nat.ptr(lims), capacity, nat.ptr(corpus.dewi32),
                                             nat.ptr(corpus.ent32), ETA, 0.0, nat.ptr(rows), nat.ptr(sims), nat.ptr(scores),
                                             nat.stream_ptr()))
        return rows.cpu().numpy(), sims.cpu().numpy(), scores.cpu().numpy()

    rows, sims, scores = collect(full, total)                      # the protocol as it is meant: the Python layer's answer
    assert np.array_equal(rows[:total], want[1]) and np.array_equal(_bits(scores[:total]), _bits(want[2]))
    assert np.all(rows[total:] == -7) and np.all(sims[total:] == -7.0) and np.all(scores[total:] == -7.0)
    cap = total - 5                                                # a short buffer: the tail is dropped, nothing beyond it written
    rows, sims, scores = collect(full, cap)
    assert np.array_equal(rows[:cap], want[1][:cap]) and np.all(rows[cap:] == -7) and np.all(scores[cap:] == -7.0)
    short = full.copy()                                            # query 1 is given 3 places fewer than it needs
    short[2:] -= 3
    rows, sims, scores = collect(short, total)
    assert np.array_equal(rows[short[1]:short[2]], want[1][full[1]:full[2] - 3])       # its first rows, and not a place more:
    assert np.array_equal(rows[short[2]:short[3]], want[1][full[2]:full[3]])           # query 2's segment is intact
    assert np.all(rows[short[-1]:] == -7)
    zero = np.zeros(nq + 1, dtype=np.int64)                        # lims that hold nothing: nothing is written
    rows, sims, scores = collect(zero, total)
    assert np.all(rows == -7) and np.all(sims == -7.0)

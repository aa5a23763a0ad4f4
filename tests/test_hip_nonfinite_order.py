"""GPU: where rows with a non-finite adjusted score end up, on every search route, against the oracle.

A zero embedding of a cosine corpus is stored as a NaN row (no guard, as in the reference); an l2 corpus can hold NaN rows
as they are; a payload value can be NaN.  The reference keeps such rows in the candidate cut and in the top k (NumPy's
partition ranks NaN as the largest value) and its final ``argsort(-adjusted)`` sorts them to the END (backends.py:468-471).
Every case plants FEWER than k such rows next to tile and row boundaries and asserts

* ``check_batch`` (tests/parity.py): the NaN scores form the tail, the tail holds the oracle's rows, and the numbers in
  front of it are the oracle's (id for id on decisive queries);
* explicitly: numbers first, NaN tail, tail set == the planted rows (== the oracle's NaN rows).

The shapes are the smallest at which each route exists; the route is asserted with ``scan_kernel_name``.

Decisive floors come from the oracle alone (``python scripts/calibrate_parity_floors.py``, section "non-finite order"); the
counts it prints for the seeds used here, and the floors asserted (all below the counts, none zero):

  one query fp32, 4 queries per (dim, k)    cosine 256: 4 4 4; 100: 4 4 3; 10: 4 4 4 at k = 5 / 40 / 150
                                            l2     256: 4 4 2; 100: 4 4 2; 10: 4 4 4        floors 0.75 / 0.5 / 0.25
  one query bf16, k = 10                    4 of 4 at both widths                            floor 0.75
  batches, 8 queries of each go to the oracle   8 of 8 on all five routes                    floor 0.6
  one list / per-query lists                6 of 6 queries (each compared twice)             at least 8 of 12
  shards                                    4 of 4 at k = 10 and at k = 200                  floors 0.75 / 0.25
  NaN dewi                                  4 of 4 (one query), 8 of 8 (batch)               floors 0.75 / 0.6
  large k (n = 3000, k = 1025)              0 of 2: with a thousand results some adjacent pair is always closer than the
                                            gap, so ``compare_query`` is called directly (near-tie rules, which hold the NaN
                                            tail to the oracle's rows all the same) next to the explicit assertions
"""
import numpy as np
import pytest

import dewi_oracle as orc
from parity import check_batch, compare_query, device_prepared_queries

pytestmark = pytest.mark.gpu

ETA, PREF = 0.3, 0.0
TOL_BF16 = dict(gap=1e-6, score_tol=1e-5, prepared=True, exact_gaps=False)
# floors below the oracle-only counts of scripts/calibrate_parity_floors.py (never zero)
ONE_QUERY_FLOOR = {5: 0.75, 40: 0.5, 150: 0.25}
BATCH_FLOOR = 0.6


# ------------------------------------------------------------------------------------------------------------ inputs (CPU)
def planted_rows(n, count, seed):
    """``count`` rows to make non-finite: the first and the last row, the rows on both sides of a 32-row tile boundary and of a
    64-row one, then random ones."""
    fixed = [0, n - 1, 31, 32, 63, 64, n - 2]
    rs = np.random.RandomState(seed)
    rest = [int(r) for r in rs.permutation(n) if r not in fixed]
    return sorted((fixed + rest)[:count])


def corpus(n, dim, space, seed, n_bad, b=4):
    """(raw rows with the planted rows zero (cosine) / NaN (l2), payload columns, queries, planted rows)."""
    raw = orc.synth_corpus(n, dim, seed=seed)
    bad = planted_rows(n, n_bad, seed)
    raw[bad] = 0.0 if space == "cosine" else np.nan
    cols = orc.synth_payload_columns(n, seed=seed)
    Q = orc.synth_queries(b, dim, seed=seed + 1)
    return raw, cols, Q, bad


def soa(cols):
    return orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])


# ------------------------------------------------------------------------------------------------------------ checks
def assert_numbers_then_nan_tail(ids, sc, planted, label=""):
    """Every row of the batch: numbers first, then a NaN tail whose ids are exactly ``planted`` (rows, or one list of rows per
    query)."""
    k = ids.shape[1]
    per_query = len(planted) > 0 and isinstance(planted[0], (list, tuple, set))
    for j in range(ids.shape[0]):
        want = set(planted[j] if per_query else planted)
        z = len(want)
        assert z < k
        nan = np.isnan(sc[j])
        assert not nan[: k - z].any() and nan[k - z:].all(), f"{label} query {j}: NaN scores at {np.nonzero(nan)[0].tolist()}, want the last {z}"
        assert set(ids[j, k - z:].tolist()) == want, f"{label} query {j}: tail {ids[j, k - z:].tolist()} != planted {sorted(want)}"
        assert np.all(sc[j, : k - z - 1] >= sc[j, 1: k - z])


def check(E, Q, dewi32, ent32, k, eta, pref, space, ids, sc, planted, floor, label="", **kw):
    assert_numbers_then_nan_tail(ids, sc, planted, label)
    return check_batch(E, Q, dewi32, ent32, k, eta, pref, space, ids, sc, min_decisive_frac=floor, **kw)


def _eng():
    from dewi import _engine as eng
    return eng


def _device(raw, cols, space="cosine", **kw):
    return _eng().DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space=space, **kw)


# ------------------------------------------------------------------------------------------------------------ one query
# (prefix, suffix) of the kernel's name; the last template argument of scan_short_rows_any says whether rows are odd
# (not whole 16-byte units)
ONE_QUERY_ROUTES = {256: ("scan_rows_f32", ""), 100: ("scan_short_rows_any<", "false>"), 10: ("scan_short_rows_any<", "true>")}


@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [256, 100, 10])
def test_one_query_f32(dim, space):
    """n = 300: the tuned kernel (256 columns), rows sharing a wave (100), odd rows (10); k = 5 / 40 / 150: workgroup lists,
    wave lists, dense keys.  Three planted rows at k = 5, seven above."""
    n = 300
    for k in (5, 40, 150):
        raw, cols, Q, bad = corpus(n, dim, space, seed=dim + k, n_bad=3 if k == 5 else 7)
        c = _device(raw, cols, space)
        name = c.scan_kernel_name(1, k)
        assert name.startswith(ONE_QUERY_ROUTES[dim][0]) and name.endswith(ONE_QUERY_ROUTES[dim][1]), name
        E = c.emb.cpu().numpy()
        assert np.isnan(E[bad]).all() and not np.isnan(np.delete(E, bad, axis=0)).any()
        got = [c.search(q, k, ETA, PREF) for q in Q]
        ids, sc = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
        check(E, Q, *soa(cols), k, ETA, PREF, space, ids, sc, bad, ONE_QUERY_FLOOR[k], f"dim {dim} k {k} {space}")


def test_one_query_large_k_global_select():
    """k = 1025 (c = 2050 > 2048): ``select_rerank_large_kernel``.  With more than a thousand results some adjacent pair is
    always closer than the gap, so no query is decisive: the near-tie rules of tests/parity.py (which hold the NaN tail to the
    oracle's rows all the same) and the explicit assertions."""
    n, dim, k = 3000, 64, 1025
    raw, cols, Q, bad = corpus(n, dim, "cosine", seed=71, n_bad=9, b=2)
    c = _device(raw, cols)
    E = c.emb.cpu().numpy()
    dewi32, ent32 = soa(cols)
    for j in range(2):
        ids, sc = c.search(Q[j], k, ETA, 0.1)
        assert_numbers_then_nan_tail(ids, sc, bad, "k 1025")
        decisive, msg = compare_query(E, Q[j], dewi32, ent32, k, ETA, 0.1, "cosine", ids[0], sc[0])
        assert msg is None, msg
        want_ids, want_sc = orc.search(E, Q[j], dewi32, ent32, k, ETA, 0.1)
        assert np.mean(ids[0, : k - 9] == want_ids[: k - 9]) > 0.98            # positions agree except at near-tie swaps


ONE_QUERY_BF16_ROUTES = {256: "scan_rows_bf16", 100: "scan_short_rows_any<1,"}


@pytest.mark.parametrize("dim", [256, 100])
def test_one_query_bf16(dim):
    n, k = 300, 10
    raw, cols, Q, bad = corpus(n, dim, "cosine", seed=dim + 3, n_bad=4)
    c = _device(raw, cols).to_bf16()
    name = c.scan_kernel_name(1, k)
    assert name.startswith(ONE_QUERY_BF16_ROUTES[dim]), name
    Eb = c.emb.float().cpu().numpy()
    assert np.isnan(Eb[bad]).all()
    got = [c.search(q, k, ETA, PREF) for q in Q]
    ids, sc = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    check(Eb, device_prepared_queries(Q), *soa(cols), k, ETA, PREF, "cosine", ids, sc, bad, 0.75, f"bf16 dim {dim}", **TOL_BF16)


# ------------------------------------------------------------------------------------------------------------ batches
# the corpus sizes of PLANTED_ROUTES in tests/test_hip_dense_neighbourhoods.py: (n, dim, b, element type, space, kernel)
BATCH_ROUTES = {
    "bf16-256query": (66_000, 256, 40, "bf16", "cosine", "mfma_scan_bf16_s16"),
    "bf16-depth": (66_000, 256, 32, "bf16", "cosine", "mfma_scan_f32<true"),
    "bf16-depth-1024": (65_600, 1024, 8, "bf16", "cosine", "mfma_scan_f32<true"),
    "f32-depth": (66_000, 128, 32, "f32", "cosine", "mfma_scan_f32<false"),
    "f32-depth-l2": (66_000, 256, 12, "f32", "l2", "mfma_scan_f32<false"),     # (l2 takes the pass from 256 columns on)
}
BATCH_K = 10
BATCH_CHECKED = 8          # queries of a batch that go to the oracle (every query gets the explicit assertions)


def batch_case(route):
    n, dim, b, elem, space, kernel = BATCH_ROUTES[route]
    raw, cols, Q, bad = corpus(n, dim, space, seed=dim + b, n_bad=5, b=b)
    return raw, cols, Q, bad, elem, space, kernel


@pytest.mark.parametrize("route", list(BATCH_ROUTES))
def test_batches_on_the_matrix_cores(route):
    import torch
    raw, cols, Q, bad, elem, space, kernel = batch_case(route)
    c = _device(raw, cols, space)
    if elem == "bf16":
        c = c.to_bf16()
    b = Q.shape[0]
    assert c.scan_kernel_name(b, BATCH_K).startswith(kernel), c.scan_kernel_name(b, BATCH_K)
    ids_d, sc_d = c.search_device(torch.from_numpy(Q).cuda(), BATCH_K, ETA, 0.1)
    ids, sc = ids_d.cpu().numpy(), sc_d.cpu().numpy()
    assert ids.min() >= 0
    assert_numbers_then_nan_tail(ids, sc, bad, route)
    sel = np.linspace(0, b - 1, BATCH_CHECKED).astype(int)
    dewi32, ent32 = soa(cols)
    if elem == "bf16":
        E, Qo, kw = c.emb.float().cpu().numpy(), device_prepared_queries(Q[sel]), TOL_BF16
    else:
        E, Qo, kw = c.emb.cpu().numpy(), Q[sel], dict(exact_gaps=False)
    check_batch(E, Qo, dewi32, ent32, BATCH_K, ETA, 0.1, space, ids[sel], sc[sel], min_decisive_frac=BATCH_FLOOR, **kw)


# ------------------------------------------------------------------------------------------------------------ lists and probes
def test_one_list_filter_and_per_query_filters():
    n, dim, k = 3000, 96, 10
    raw, cols, Q, bad = corpus(n, dim, "cosine", seed=96, n_bad=5, b=6)
    c = _device(raw, cols)
    E = c.emb.cpu().numpy()
    dewi32, ent32 = soa(cols)
    rs = np.random.RandomState(4)
    masks = rs.rand(6, n) < 0.4
    masks[:, bad[:3]] = True                                       # three planted rows in every list,
    masks[:, bad[3:]] = False
    masks[1, bad[3]] = True                                        # ... a fourth in list 1
    lists = [c.search(Q[j:j + 1], k, ETA, PREF, filter=c.make_filter(masks[j])) for j in range(6)]
    ids_q, sc_q = c.search(Q, k, ETA, PREF, filter=c.make_query_filters(masks))
    n_dec = 0
    for j in range(6):
        rows = np.nonzero(masks[j])[0]
        planted = [r for r in bad if masks[j, r]]
        for ids, sc in (lists[j], (ids_q[j:j + 1], sc_q[j:j + 1])):
            assert_numbers_then_nan_tail(ids, sc, planted, f"list {j}")
            pos = np.searchsorted(rows, ids[0])
            assert np.array_equal(rows[pos], ids[0]), f"query {j}: an id outside its list"
            decisive, msg = compare_query(E[rows], Q[j], dewi32[rows], ent32[rows], k, ETA, PREF, "cosine", pos, sc[0])
            assert msg is None, f"query {j}: {msg}"
            n_dec += int(decisive)
    assert n_dec >= 8, n_dec                                       # of 12 comparisons (the oracle alone: 12)


def test_ivf_probe():
    from dewi.ivf import IVFIndex
    n, dim, k = 3000, 96, 10
    raw, cols, Q, bad = corpus(n, dim, "cosine", seed=97, n_bad=4, b=6)
    ivf = IVFIndex(dim, "cosine", nlist=16, train_iters=3)
    ivf.add_batch_columns([f"d{i}" for i in range(n)], raw, cols)
    ivf.build()
    E = orc.build_matrix(raw)
    dewi32, ent32 = soa(cols)
    cells = ivf.probe(Q, 4)
    ids, sc = ivf.search_batch(Q, k, ETA, PREF, nprobe=4)
    n_dec = n_nan = 0
    for j in range(6):
        mask = np.isin(ivf.cell_of_row, cells[j])
        rows = np.nonzero(mask)[0]
        planted = [r for r in bad if mask[r]]                      # the planted rows of the probed cells (a NaN row lies in some cell)
        n_nan += len(planted)
        assert_numbers_then_nan_tail(ids[j:j + 1], sc[j:j + 1], planted, f"probe {j}")
        pos = np.searchsorted(rows, ids[j])
        assert np.array_equal(rows[pos], ids[j])
        decisive, msg = compare_query(E[rows], Q[j], dewi32[rows], ent32[rows], k, ETA, PREF, "cosine", pos, sc[j])
        assert msg is None, f"query {j}: {msg}"
        n_dec += int(decisive)
    assert n_dec >= 4 and n_nan >= 1, (n_dec, n_nan)


# ------------------------------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize("n,dim,k,bounds", [(3000, 96, 10, [0, 1000, 1015, 3000]),                      # three shards, merge in LDS
                                            (6000, 64, 200, [0, 750, 1500, 2250, 3000, 3750, 4500, 5250, 6000])],   # eight, global rank-merge
                         ids=["3-shards-k10", "8-shards-k200"])
def test_shards_and_merge(n, dim, k, bounds):
    import torch
    eng = _eng()
    raw, cols, Q, bad = corpus(n, dim, "cosine", seed=dim + k, n_bad=7, b=4)
    whole = _device(raw, cols)
    qd = torch.from_numpy(Q).cuda()
    c = min(2 * k, n)
    lists = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sub = {key: v[lo:hi] for key, v in cols.items()}
        lists.append(_device(raw[lo:hi], sub, id_offset=lo).candidates_device(qd, c))
    ids_d, sc_d = eng.merge_rerank_device(torch.stack(lists), c, k, ETA, PREF)
    ids, sc = ids_d.cpu().numpy(), sc_d.cpu().numpy()
    E = whole.emb.cpu().numpy()
    check(E, Q, *soa(cols), k, ETA, PREF, "cosine", ids, sc, bad, 0.75 if k == 10 else 0.25, f"{len(bounds) - 1} shards")


# ------------------------------------------------------------------------------------------------------------ ANN rule
@pytest.mark.parametrize("space,kind", [("cosine", "ip"), ("cosine", "one_minus_dist"), ("l2", "one_minus_dist"),
                                        ("l2", "inv_one_plus_dist"), ("cosine", "inv_one_plus_dist")])
def test_ann_rule_candidates_equal_k(space, kind):
    """``candidates=k``: the k nearest rows (NaN similarities on top, as in the cut) blended with the library's similarity and
    ordered by ``oracle.ann_rerank`` (stable ``argsort(-adj)``: NaN last as well)."""
    n, dim, k, eta, pref = 3000, 96, 10, 0.4, 0.2
    raw, cols, Q, bad = corpus(n, dim, space, seed=33, n_bad=3, b=5)
    c = _device(raw, cols, space)
    E = c.emb.cpu().numpy()
    ids, sc = c.search(Q, k, eta, pref, candidates=k, similarity=kind)
    assert_numbers_then_nan_tail(ids, sc, bad, kind)
    for j in range(Q.shape[0]):
        qp = orc.prepare_query(Q[j], space)
        s = orc.similarities(E, qp, space)
        nn = np.argsort(-np.where(np.isnan(s), np.inf, s.astype(np.float64)), kind="stable")[:k]
        sim = s[nn] if kind == "ip" else orc.ann_similarity(orc.ann_library_distance(E, qp, space)[nn], kind)
        with np.errstate(invalid="ignore"):
            want_ids, want_sc = orc.ann_rerank(nn, sim.astype(np.float64), cols["dewi"], cols["ht_mean"], cols["hi_mean"], eta, pref)
        assert np.isnan(want_sc[k - 3:]).all() and set(want_ids[k - 3:].tolist()) == set(bad)
        assert np.array_equal(ids[j, : k - 3], want_ids[: k - 3]), (j, ids[j], want_ids)
        assert np.allclose(sc[j, : k - 3], want_sc[: k - 3], rtol=0, atol=1e-5 * max(1.0, float(np.abs(want_sc[: k - 3]).max())))


# ------------------------------------------------------------------------------------------------------------ payload NaN
def payload_case(n, dim, b, seed):
    """Queries that are noisy copies of rows r_j; the dewi value of every r_j is NaN: a NaN adjusted score on a row with a
    finite similarity (about 1) inside the cut of query j."""
    raw = orc.synth_corpus(n, dim, seed=seed)
    cols = orc.synth_payload_columns(n, seed=seed)
    rs = np.random.RandomState(seed + 5)
    rows = rs.choice(n, b, replace=False)
    Q = (raw[rows] + 0.02 * rs.randn(b, dim)).astype(np.float32)
    cols = dict(cols, dewi=cols["dewi"].copy())
    cols["dewi"][rows] = np.nan
    return raw, cols, Q, rows


def _oracle_tails(E, Q, dewi32, ent32, k, eta, pref, space="cosine", prepared=False):
    out = []
    for q in Q:
        search = orc.search_prepared if prepared else orc.search
        with np.errstate(invalid="ignore"):
            ids, sc = search(E, q, dewi32, ent32, k, eta, pref, space)
        out.append(ids[np.isnan(sc)].tolist())
    return out


def test_nan_dewi_one_query():
    n, dim, k = 300, 100, 5
    raw, cols, Q, rows = payload_case(n, dim, 4, seed=8)
    c = _device(raw, cols)
    E = c.emb.cpu().numpy()
    dewi32, ent32 = soa(cols)
    got = [c.search(q, k, ETA, PREF) for q in Q]
    ids, sc = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    tails = _oracle_tails(E, Q, dewi32, ent32, k, ETA, PREF)
    assert all(int(rows[j]) in tails[j] for j in range(4))
    check(E, Q, dewi32, ent32, k, ETA, PREF, "cosine", ids, sc, tails, 0.75, "NaN dewi")


def test_nan_dewi_batched():
    import torch
    n, dim, b, k = 66_000, 128, 32, 10
    raw, cols, Q, rows = payload_case(n, dim, b, seed=9)
    c = _device(raw, cols)
    assert c.scan_kernel_name(b, k).startswith("mfma_scan_f32<false")
    ids_d, sc_d = c.search_device(torch.from_numpy(Q).cuda(), k, ETA, PREF)
    ids, sc = ids_d.cpu().numpy(), sc_d.cpu().numpy()
    E = c.emb.cpu().numpy()
    dewi32, ent32 = soa(cols)
    sel = np.linspace(0, b - 1, BATCH_CHECKED).astype(int)
    tails = _oracle_tails(E, Q[sel], dewi32, ent32, k, ETA, PREF)
    assert all(int(rows[j]) in t for j, t in zip(sel, tails))
    check(E, Q[sel], dewi32, ent32, k, ETA, PREF, "cosine", ids[sel], sc[sel], tails, BATCH_FLOOR, "NaN dewi, batch", exact_gaps=False)
    for j in range(b):                                             # every query: its own row last, with a NaN score
        nan = np.isnan(sc[j])
        assert nan.any() and nan[k - int(nan.sum()):].all() and int(rows[j]) in ids[j, nan].tolist()


def test_golden_nan_rows(golden):
    """tests/golden/g7_nan_rows.npz: the REFERENCE's own results (ExactIndex) on a corpus with zero rows and a NaN dewi value.
    Numbers id for id and to 1e-5, NaN tail as a set."""
    g = golden("g7_nan_rows.npz")
    for name in [str(s) for s in g["cases"]]:
        space = "l2" if name.startswith("l2") else "cosine"
        raw, q = g[f"{name}__raw"], g[f"{name}__query"]
        k, eta, pref = int(g[f"{name}__k"]), float(g[f"{name}__eta"]), float(g[f"{name}__pref"])
        cols = dict(dewi=g[f"{name}__dewi"], ht_mean=g[f"{name}__ht_mean"], hi_mean=g[f"{name}__hi_mean"])
        c = _device(raw, cols, space)
        ids, sc = c.search(q, k, eta, pref)
        want_ids, want_sc = g[f"{name}__ids"], g[f"{name}__scores"]
        z = int(np.isnan(want_sc).sum())
        assert z > 0 and np.isnan(want_sc[k - z:]).all()
        assert np.isnan(sc[0, k - z:]).all() and not np.isnan(sc[0, : k - z]).any(), name
        assert np.array_equal(ids[0, : k - z], want_ids[: k - z]), name
        assert np.allclose(sc[0, : k - z], want_sc[: k - z], rtol=0, atol=1e-5 * max(1.0, float(np.abs(want_sc[: k - z]).max()) if z < k else 1.0))
        if not bool(g[f"{name}__tail_is_a_choice"]):
            assert set(ids[0, k - z:].tolist()) == set(want_ids[k - z:].tolist()), name
        else:                                                       # k below the NaN count: any k of the NaN candidates
            assert set(ids[0].tolist()) <= set(g[f"{name}__nan_candidates"].tolist()), name

"""GPU parity tests of the search path (A1-A5), all through the C ABI.

Each test builds the same seeded inputs for the HIP path and the CPU oracle
(oracle/dewi_oracle.py, pinned to the reference by tests/test_oracle_golden.py) and
compares with tests/parity.py; golden vectors produced by the reference itself are
checked directly as well.
"""
import json

import numpy as np
import pytest

import dewi_oracle as orc
from parity import check_batch, compare_query

pytestmark = pytest.mark.gpu


def _engine():
    from dewi import _engine
    return _engine


def _corpus(E_raw, cols, space="cosine", normalize=None):
    eng = _engine()
    return eng.DeviceCorpus.from_host(E_raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space, normalize=normalize)


def test_library_reports_mi355x():
    import ctypes
    from dewi import _native as nat
    lib = nat.load_library()
    cu, wave, mem = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    nat.check(lib.dewi_device_info(ctypes.byref(cu), ctypes.byref(wave), ctypes.byref(mem)))
    assert wave.value == 64 and cu.value >= 64 and mem.value > (1 << 30)


def test_normalize_rows_matches_oracle():
    rs = np.random.RandomState(0)
    for n, d in ((7, 8), (100, 128), (33, 10), (257, 768), (5, 1000)):
        raw = (rs.randn(n, d) * rs.uniform(0.1, 10)).astype(np.float32)
        cols = orc.synth_payload_columns(n, seed=1)
        c = _corpus(raw, cols)
        got = c.emb.cpu().numpy()
        want = orc.build_matrix(raw)
        assert np.allclose(got, want, rtol=0, atol=2e-7), (n, d, np.abs(got - want).max())
        # the device divides by the float64-summed norm rounded once, NumPy by an fp32 dot product's root: <= 2 ulp apart
        assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want))), (n, d)
        assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # zero row -> NaN row, like the reference (no guard)
    raw = rs.randn(4, 16).astype(np.float32)
    raw[2] = 0
    got = _corpus(raw, orc.synth_payload_columns(4, seed=1)).emb.cpu().numpy()
    assert np.all(np.isnan(got[2])) and not np.any(np.isnan(got[[0, 1, 3]]))


def test_payload_soa_bit_exact():
    cols = orc.synth_payload_columns(1000, seed=9)
    c = _corpus(np.random.RandomState(1).randn(1000, 8).astype(np.float32), cols)
    d32, e32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    assert np.array_equal(c.dewi32.cpu().numpy(), d32)
    assert np.array_equal(c.ent32.cpu().numpy(), e32)


def test_g1_reference_golden_through_the_api(golden):
    """tests/test_index.py shape, via ExactIndex.add/build/search, against the reference's outputs."""
    from dewi.index import ExactIndex, Payload
    g = golden("g1_test_index_shape.npz")
    n = g["E"].shape[0]
    idx = ExactIndex(dim=g["E"].shape[1], space="cosine")
    pay = [Payload(**{k: float(g[f"p_{k}"][i]) for k in orc.PAYLOAD_KEYS}) for i in range(n)]
    for i in range(n):
        idx.add(f"doc_{i}", g["E"][i], pay[i])
    idx.build()
    k = int(g["k"])
    dewi32, ent32 = orc.payload_soa(g["p_dewi"], g["p_ht_mean"], g["p_hi_mean"])
    mism = 0
    for a, eta in enumerate(g["etas"]):
        for b, pref in enumerate(g["prefs"]):
            for j, q in enumerate(g["Q"]):
                res = idx.search(q, k=k, eta=float(eta), entropy_pref=float(pref))
                assert len(res) == k
                assert all(isinstance(r[0], str) and isinstance(r[1], float) and r[2] is pay[int(r[0][4:])] for r in res)
                ids = np.array([int(r[0][4:]) for r in res])
                sc = np.array([r[1] for r in res], np.float32)
                decisive, msg = compare_query(g["stored"], q, dewi32, ent32, k, float(eta), float(pref), "cosine", ids, sc)
                assert msg is None, (eta, pref, j, msg)
                if decisive:
                    assert np.array_equal(ids, g["ids"][a, b, j])
                    assert np.allclose(sc, g["scores"][a, b, j], rtol=0, atol=1e-5)
                else:
                    mism += 1
    assert mism <= 4


def test_g2_c1_10k_768_golden(golden):
    """Config C1 (10K x 768, k=10, eta=0.3): fast row-per-wave kernel vs the reference's outputs."""
    g = golden("g2_c1_10k_768.npz")
    n, d, k, eta = int(g["n"]), int(g["d"]), int(g["k"]), float(g["eta"])
    raw = orc.synth_corpus(n, d, seed=int(g["corpus_seed"]))
    cols = orc.synth_payload_columns(n, seed=int(g["corpus_seed"]))
    Q = orc.synth_queries(g["ids"].shape[0], d, seed=int(g["query_seed"]))
    c = _corpus(raw, cols)
    ids, sc = c.search(Q, k, eta, 0.0)            # one batched call (NQ=4 passes)
    ids1 = np.stack([c.search(Q[j], k, eta, 0.0)[0][0] for j in range(8)])   # batch-1 kernel
    assert np.array_equal(ids1, ids[:8])
    E = orc.build_matrix(raw)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    n_decisive = check_batch(E, Q, dewi32, ent32, k, eta, 0.0, "cosine", ids, sc, min_decisive_frac=0.9)
    exact = sum(int(np.array_equal(ids[j], g["ids"][j])) for j in range(Q.shape[0]))
    assert exact >= n_decisive
    assert np.max(np.abs(sc[ids == g["ids"]] - g["scores"][ids == g["ids"]])) <= 1e-5


def test_g3_edge_cases(golden, golden_dir):
    g = golden("g3_edge_cases.npz")
    meta = json.loads((golden_dir / "g3_edge_cases.json").read_text())
    cols = {k: g[f"p_{k}"] for k in orc.PAYLOAD_KEYS}
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    c_cos = _corpus(g["E"], cols, "cosine")
    c_l2 = _corpus(g["E"], cols, "l2")
    assert np.array_equal(c_l2.emb.cpu().numpy(), g["E"])        # l2 keeps raw rows
    names = sorted({key.split("__")[0] for key in g.files if "__" in key})
    for name in names:
        q, k = g[f"{name}__q"], int(g[f"{name}__k"])
        eta, pref = float(g[f"{name}__eta"]), float(g[f"{name}__pref"])
        space = "l2" if name.startswith("l2") else "cosine"
        corpus = c_l2 if space == "l2" else c_cos
        E = g["E"] if space == "l2" else g["stored_cos"]
        ids, sc = corpus.search(q, k, eta, pref)
        if name == "zero_query":
            # Every similarity is exactly 0, so WHICH 2k rows survive the cut is a tie artefact (NumPy's
            # introselect in the reference; lowest rows first here) and the scores follow that choice.
            # What is defined: the blend over the chosen candidates.  Ours are rows 0..2k-1.
            adj = np.float32(1 - eta) * np.float32(0) + np.float32(eta) * dewi32[: 2 * k]
            want = np.argsort(-adj, kind="stable")[:k]
            assert ids[0].tolist() == want.tolist() and np.array_equal(sc[0], adj[want])
            ref_adj = np.float32(eta) * dewi32[g[f"{name}__ids"]]      # the reference obeys the same formula
            assert np.array_equal(ref_adj.astype(np.float32), g[f"{name}__scores"])
            continue
        decisive, msg = compare_query(E, q, dewi32, ent32, k, eta, pref, space, ids[0], sc[0])
        assert msg is None, (name, msg)
        if decisive:
            assert np.array_equal(ids[0], g[f"{name}__ids"]), name
            tol = 1e-5 * max(1.0, float(np.abs(g[f"{name}__scores"]).max()))
            assert np.allclose(sc[0], g[f"{name}__scores"], rtol=0, atol=tol), name
    # k > N -> ValueError with NumPy's message; k == 0 -> empty
    with pytest.raises(ValueError, match="out of bounds"):
        c_cos.search(g["k_eq_n__q"], meta["n"] + 1, 0.3, 0.0)
    ids, sc = c_cos.search(g["k_eq_n__q"], 0, 0.3, 0.0)
    assert ids.shape == (1, 0) and sc.shape == (1, 0)


@pytest.mark.parametrize("dim", [4, 8, 10, 12, 16, 36, 64, 100, 128, 132, 252, 256, 260, 384, 512, 768, 1000, 1024, 1280, 1536,
                                 1792, 2048, 2304, 3072, 4096, 4100])
def test_dimension_sweep_vs_oracle(dim):
    """Every row-kernel variant: the tuned widths (dim = 256*U), the any-width kernels of scan_any.hpp — short rows sharing a
    wave (dim <= 128: 1, 2, 4 ... 32 lanes per row, with idle lanes at 12 / 36 / 100), one row per step with a predicated tail
    (132 ... 4096: every instantiated units-per-lane count, 1792 and 2304 on a padded one), two queries per pass beyond
    2048 columns — the form of those kernels for rows that are not whole units (dim % 4 != 0: 10; tests/test_hip_odd_rows.py
    has the sweep of those) and the generic kernel (beyond 4096 columns: 4100)."""
    n = 3001 if dim <= 1024 else 1500
    raw = orc.synth_corpus(n, dim, seed=dim)
    cols = orc.synth_payload_columns(n, seed=dim)
    Q = orc.synth_queries(5, dim, seed=dim + 1)      # 5 = one NQ=4 pass + one NQ=1 pass
    c = _corpus(raw, cols)
    E = c.emb.cpu().numpy()                             # same stored rows on both sides
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    for k, eta, pref in ((1, 0.3, 0.0), (10, 0.3, 0.0), (10, 0.7, -0.5), (100, 0.25, 0.3), (150, 0.5, 0.0)):
        ids, sc = c.search(Q, k, eta, pref)          # k=150 -> c=300 > 256: dense-key path
        check_batch(E, Q, dewi32, ent32, k, eta, pref, "cosine", ids, sc, min_decisive_frac=0.8 if k <= 10 else 0.6)


@pytest.mark.parametrize("dim", [16, 100, 128, 384, 768, 1000, 3072])
def test_l2_space_vs_oracle(dim):
    n = 2000 if dim <= 1024 else 1000
    rs = np.random.RandomState(dim)
    raw = (rs.randn(n, dim) * 0.5).astype(np.float32)
    cols = orc.synth_payload_columns(n, seed=3)
    Q = (rs.randn(5, dim) * 0.5).astype(np.float32)
    c = _corpus(raw, cols, "l2")
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    for k in (10, 40, 150):       # per-workgroup lists, per-wave lists, dense keys
        ids, sc = c.search(Q, k, 0.3, 0.0)
        check_batch(raw, Q, dewi32, ent32, k, 0.3, 0.0, "l2", ids, sc, min_decisive_frac=0.8 if k <= 10 else 0.5)


def test_ties_prefer_lower_row_and_zero_query():
    """Duplicate rows tie exactly; the device order is (sim desc, row asc) — deterministic, unlike
    the reference's introselect artefact (SURVEY.md §7 hard part (i))."""
    rs = np.random.RandomState(5)
    base = rs.randn(4, 256).astype(np.float32)
    raw = np.concatenate([base, base, base], axis=0)           # rows i, i+4, i+8 identical
    cols = {k: np.zeros(12) for k in orc.PAYLOAD_KEYS}
    c = _corpus(raw, cols)
    ids, sc = c.search(base[1], 3, 0.0, 0.0)
    assert ids[0].tolist() == [1, 5, 9]
    assert np.allclose(sc[0], 1.0, atol=1e-6)
    ids, sc = c.search(np.zeros(256, np.float32), 5, 0.0, 0.0)  # all sims exactly 0
    assert ids[0].tolist() == [0, 1, 2, 3, 4] and np.all(sc[0] == 0)


def test_nan_rows_rank_last_like_numpy():
    """A zero-norm row becomes NaN at build (reference has no guard).  NumPy's partition ranks NaN as the largest value,
    so the row stays in the cut and in the top k; the reference's final ``argsort(-adjusted)`` then sorts it to the END
    (backends.py:468-471): the numbers come first, id for id as the oracle has them, the NaN row last."""
    rs = np.random.RandomState(6)
    raw = rs.randn(300, 256).astype(np.float32)
    raw[17] = 0
    cols = orc.synth_payload_columns(300, seed=6)
    c = _corpus(raw, cols)
    q = rs.randn(256).astype(np.float32)
    ids, sc = c.search(q, 5, 0.3, 0.0)
    assert ids[0, 4] == 17 and np.isnan(sc[0, 4]) and not np.any(np.isnan(sc[0, :4]))
    E = c.emb.cpu().numpy()
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    want_ids, want_sc = orc.search(E, q, dewi32, ent32, 5, 0.3, 0.0)
    assert want_ids[4] == 17 and np.isnan(want_sc[4])
    decisive, msg = compare_query(E, q, dewi32, ent32, 5, 0.3, 0.0, "cosine", ids[0], sc[0])
    assert msg is None and decisive                       # (decisive by the oracle alone: scripts/calibrate_parity_floors.py)
    assert ids[0, :4].tolist() == want_ids[:4].tolist()


def test_sharded_candidates_and_merge_equal_single_device():
    """Row (e): per-shard top-2k records + merge == the unsharded search (same GPU, 3 ragged shards)."""
    eng = _engine()
    import torch
    n, d, k, eta, pref = 5000, 768, 10, 0.3, 0.2
    raw = orc.synth_corpus(n, d, seed=77)
    cols = orc.synth_payload_columns(n, seed=77)
    Q = orc.synth_queries(6, d, seed=78)
    whole = _corpus(raw, cols)
    ids_ref, sc_ref = whole.search(Q, k, eta, pref)
    bounds = [0, 1700, 1715, n]                       # middle shard has only 15 rows (< 2k = 20)
    c = min(2 * k, n)
    lists = []
    qd = torch.from_numpy(Q).cuda()
    for s in range(3):
        lo, hi = bounds[s], bounds[s + 1]
        sub = {key: v[lo:hi] for key, v in cols.items()}
        shard = eng.DeviceCorpus.from_host(raw[lo:hi], sub["dewi"], sub["ht_mean"], sub["hi_mean"], "cosine", id_offset=lo)
        lists.append(shard.candidates_device(qd, c))
    recs = eng.records_to_numpy(lists[1])
    assert np.all(recs["id"][:, 15:] == -1) and np.all(recs["id"][:, :15] >= 1700)
    assert np.all(np.diff(eng.records_to_numpy(lists[0])["sim"], axis=1) <= 0)
    ids, sc = eng.merge_rerank_device(torch.stack(lists), c, k, eta, pref)
    assert np.array_equal(ids.cpu().numpy(), ids_ref)
    assert np.array_equal(sc.cpu().numpy(), sc_ref)


@pytest.mark.parametrize("n,k", [(5000, 5000), (6000, 1500), (3000, 1025)])
def test_large_k_global_memory_path(n, k):
    """k > 1024 (candidate count > 2048, up to k == N): candidates are selected and sorted in global
    memory.  The reference accepts any k <= N, so must this."""
    dim = 64
    raw = orc.synth_corpus(n, dim, seed=n)
    cols = orc.synth_payload_columns(n, seed=n)
    Q = orc.synth_queries(2, dim, seed=k)
    c = _corpus(raw, cols)
    E = c.emb.cpu().numpy()
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    ids, sc = c.search(Q, k, 0.3, 0.1)
    assert ids.shape == (2, k)
    for j in range(2):
        # with > 1000 results some adjacent pair is always closer than the gap, so the query is not "decisive":
        # the near-tie rules of tests/parity.py compare the id SET (every returned row an admissible candidate
        # carrying that row's score, no sure candidate left out), and positions must agree except at swaps
        decisive, msg = compare_query(E, Q[j], dewi32, ent32, k, 0.3, 0.1, "cosine", ids[j], sc[j])
        assert msg is None, (j, msg)
        ref_ids, ref_sc = orc.search(E, Q[j], dewi32, ent32, k, 0.3, 0.1)
        if k == n:
            assert sorted(ids[j].tolist()) == list(range(n))                     # every row exactly once
        diff = set(ids[j].tolist()) ^ set(ref_ids.tolist())
        assert len(diff) <= 4, diff                                               # only rows at the two decision boundaries
        assert np.mean(ids[j] == ref_ids) > 0.99                                  # near-tie swaps only


def test_pipelined_searcher_equals_serial_search():
    """dewi_knn_scan / dewi_knn_finish on two streams (PipelinedSearcher) == the one-call search,
    for final results and for shard candidate records."""
    import torch
    eng = _engine()
    n, d, k = 30_000, 768, 10
    raw = orc.synth_corpus(n, d, seed=11)
    cols = orc.synth_payload_columns(n, seed=11)
    c = _corpus(raw, cols)
    Q = torch.from_numpy(orc.synth_queries(12, d, seed=12)).cuda()
    want_ids, want_sc = c.search_device(Q, k, 0.3, 0.1)
    pipe = eng.PipelinedSearcher(c, k, 0.3, 0.1, n_queries=1)
    ids = torch.empty((12, 1, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((12, 1, k), dtype=torch.float32, device="cuda")
    for j in range(12):
        pipe.submit(Q[j:j + 1], ids[j], sc[j])
    pipe.drain()
    assert torch.equal(ids[:, 0], want_ids) and torch.equal(sc[:, 0], want_sc)
    recs = torch.empty((12, 1, 2 * k, 4), dtype=torch.int32, device="cuda")
    pipe2 = eng.PipelinedSearcher(c, k, 0.3, 0.1, n_queries=1, n_candidates=2 * k)
    for j in range(12):
        pipe2.submit(Q[j:j + 1], out_records=recs[j])
    pipe2.drain()
    want = c.candidates_device(Q, 2 * k)
    assert torch.equal(recs[:, 0], want)


def test_ann_semantics_candidates_equal_k():
    """F4 / A10: candidates=k re-ranks exactly the k nearest rows (the HNSW / FAISS backends' rule,
    reference backends.py:217-240) — checked against the oracle's ann_rerank on exact neighbours."""
    n, d, k, eta, pref = 4000, 128, 10, 0.4, 0.2
    raw = orc.synth_corpus(n, d, seed=21)
    cols = orc.synth_payload_columns(n, seed=21)
    Q = orc.synth_queries(6, d, seed=22)
    c = _corpus(raw, cols)
    E = c.emb.cpu().numpy()
    ids, sc = c.search(Q, k, eta, pref, candidates=k)
    ids2k, _ = c.search(Q, k, eta, pref)
    assert not np.array_equal(ids, ids2k)                       # a different rule than the 2k cut
    for j in range(Q.shape[0]):
        s = orc.similarities(E, orc.prepare_query(Q[j]))
        nn = np.argsort(-s.astype(np.float64), kind="stable")[:k]
        want_ids, want_sc = orc.ann_rerank(nn, s[nn].astype(np.float64), cols["dewi"], cols["ht_mean"], cols["hi_mean"],
                                           eta, pref)
        assert sorted(ids[j].tolist()) == sorted(nn.tolist())   # exactly the k nearest rows
        assert np.array_equal(ids[j], want_ids), j
        assert np.allclose(sc[j], want_sc, atol=1e-5)
    with pytest.raises(ValueError, match="at least k"):
        c.search(Q, k, eta, pref, candidates=k - 1)


def _random_cases(n_cases, seed):
    rs = np.random.RandomState(seed)
    dims = [1, 3, 7, 8, 24, 33, 64, 96, 100, 128, 129, 200, 256, 384, 512, 640, 768, 1000]
    out = []
    for _ in range(n_cases):
        n = int(rs.choice([1, 2, 3, 17, 64, 255, 256, 257, 1000, 2049, 4000]))
        dim = int(rs.choice(dims))
        b = int(rs.randint(1, 10))
        k = int(rs.randint(1, min(n, 300) + 1))
        eta = float(rs.choice([0.0, 0.3, 0.5, 1.0, rs.rand()]))
        pref = float(rs.choice([0.0, -1.0, 0.5, rs.uniform(-1, 1)]))
        space = str(rs.choice(["cosine", "cosine", "l2"]))
        out.append((n, dim, b, k, eta, pref, space))
    return out


@pytest.mark.parametrize("case", _random_cases(36, seed=20261004), ids=lambda c: "n%d-d%d-b%d-k%d-%s" % (c[0], c[1], c[2], c[3], c[6]))
def test_randomised_shapes_vs_oracle(case):
    """Seeded sweep over corpus size (incl. 1, 2, 3 rows and non-multiples of every tile size), dimension (odd,
    tiny, non-multiples of 256), batch, k (up to N: candidate count clamps to N), eta / entropy_pref and space."""
    from dewi import _engine as eng
    n, dim, b, k, eta, pref, space = case
    rs = np.random.RandomState(n * 31 + dim)
    raw = (rs.randn(n, dim) * (0.5 if space == "l2" else 1.0)).astype(np.float32)
    cols = orc.synth_payload_columns(n, seed=dim)
    Q = (rs.randn(b, dim) * (0.5 if space == "l2" else 1.0)).astype(np.float32)
    c = eng.DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space)
    E = c.emb.cpu().numpy()
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    ids, sc = c.search(Q, k, eta, pref)
    assert ids.shape == (b, k) and sc.shape == (b, k) and ids.min() >= 0 and ids.max() < n
    # decisive floor calibrated on the oracle alone (scripts/calibrate_parity_floors.py): 177 of the 185 queries
    # of this sweep are decisive; the two low cases are (17 rows, dim 1: sims are +-1, all ties) and k > 200
    floor = 0.3 if (dim == 1 or k > 200) else 0.75
    check_batch(E, Q, dewi32, ent32, k, eta, pref, space, ids, sc, min_decisive_frac=floor)


@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("dim", [256, 768, 1536])
def test_eight_queries_per_pass(dim, space):
    """21 queries = 8 + 8 + 4 + 1: every queries-per-pass variant of the row-per-wave fp32 kernel in one call; the
    answers must not depend on how the batch is cut (same rows, same order of every per-row sum)."""
    from dewi import _engine as eng
    n = 3001
    rs = np.random.RandomState(dim)
    scale = 0.5 if space == "l2" else 1.0
    raw = (rs.randn(n, dim) * scale).astype(np.float32)
    cols = orc.synth_payload_columns(n, seed=dim)
    Q = (rs.randn(21, dim) * scale).astype(np.float32)
    c = eng.DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space)
    ids, sc = c.search(Q, 10, 0.3, 0.1)
    for j in (0, 7, 8, 15, 16, 19, 20):                        # one at a time: the single-query kernel
        i1, s1 = c.search(Q[j], 10, 0.3, 0.1)
        assert np.array_equal(i1[0], ids[j]) and np.array_equal(s1[0], sc[j]), j
    E = c.emb.cpu().numpy()
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    check_batch(E, Q, dewi32, ent32, 10, 0.3, 0.1, space, ids, sc, min_decisive_frac=0.9)

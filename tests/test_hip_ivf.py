"""GPU tests of ``IVFIndex``: approximate search over the rows of the probed k-means cells.

Contract: query j's answer is the reference's ExactIndex.search (src/dewi/backends.py:414-481) applied to F_j, the rows of
the ``nprobe`` cells nearest to it — bit for bit what ``ExactIndex.search(q_j, ..., filter=<mask of F_j>)`` returns, and with
``nprobe = nlist`` the exact search itself.  The corpus is clustered (64 gaussian centres), so that recall means something.
"""
import numpy as np
import pytest

import dewi_oracle as orc
from parity import compare_query, default_floor

pytestmark = pytest.mark.gpu

N, D, NLIST, K = 20000, 64, 64, 10


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


def _pair(n=N, d=D, space="cosine", seed=0, nlist=NLIST, noise=1.0, **kw):
    """(IVFIndex, ExactIndex on the same rows and payloads, queries, payload columns)."""
    from dewi.backends import ExactIndex
    from dewi.ivf import IVFIndex
    X, Q = _clustered(n, d, seed, noise)
    cols = orc.synth_payload_columns(n, seed=seed)
    ids = [f"doc_{i:07d}" for i in range(n)]
    ivf = IVFIndex(d, space, nlist=nlist, **kw)
    ivf.add_batch_columns(ids, X, cols)
    ivf.build()
    exact = ExactIndex(d, space)
    exact.add_batch_columns(ids, X, cols)
    exact.build()
    return ivf, exact, Q, cols


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _mask_of(ivf, cells):
    return np.isin(ivf.cell_of_row, cells)


# ------------------------------------------------------------------------------------------------------- 1. cell lists
@pytest.mark.parametrize("dim", [96, 50, 129])
def test_cell_lists(dim):
    n = 20011
    ivf, _, _, _ = _pair(n, dim, "cosine", seed=dim, nlist=64, train_iters=3)
    offsets, rows, g = ivf.cell_lists()
    assert g == {96: 1, 50: 2, 129: 4}[dim]
    cell = ivf.cell_of_row
    assert cell.dtype == np.int32 and cell.shape == (n,) and cell.min() >= 0 and cell.max() < 64
    assert offsets.shape == (64 * g + 1,) and offsets[0] == 0 and offsets[-1] == n
    assert np.all(np.diff(offsets.astype(np.int64)) >= 0)
    assert np.array_equal(np.sort(rows), np.arange(n, dtype=np.uint32))          # every row exactly once
    for c in range(64):
        for b in range(g):
            seg = rows[offsets[c * g + b]: offsets[c * g + b + 1]].astype(np.int64)
            want = np.nonzero((cell == c) & (np.arange(n) % g == b))[0]
            assert np.array_equal(seg, want), (c, b)                               # its segment, ascending
    assert np.array_equal(ivf.cell_sizes, np.bincount(cell, minlength=64))


def test_cell_lists_drop_bad_assignments():
    """ABI level: a row assigned outside [0, n_cells) is dropped and counted, nothing else moves."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    n, dim, cells = 5000, 50, 16
    rs = np.random.RandomState(3)
    assign = rs.randint(0, cells, n).astype(np.int32)
    bad = rs.choice(n, 7, replace=False)
    assign[bad[:4]] = cells
    assign[bad[4:]] = -1
    need = lib.dewi_ivf_lists_bytes(n, dim, 0, cells)
    buf = torch.zeros(need, dtype=torch.uint8, device="cuda")
    a = torch.from_numpy(assign).cuda()
    nat.check(lib.dewi_ivf_lists_build(0, n, dim, cells, nat.ptr(a), nat.ptr(buf), need, nat.stream_ptr()))
    words = buf.view(torch.int32).cpu().numpy().view(np.uint32)
    g = lib.dewi_ivf_buckets(dim, 0)
    bins = cells * g
    assert words[bins + 1 + n] == 7
    assert words[bins] == n - 7
    for c in range(cells):
        for b in range(g):
            seg = words[bins + 1 + words[c * g + b]: bins + 1 + words[c * g + b + 1]].astype(np.int64)
            assert np.array_equal(seg, np.nonzero((assign == c) & (np.arange(n) % g == b))[0]), (c, b)


# ------------------------------------------------------------------------------------------------------- 2. coarse step
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_probe_is_the_top_centroids(space):
    ivf, _, Q, _ = _pair(space=space, seed=1)
    C = ivf.centroids
    assert C.dtype == np.float32 and C.shape == (NLIST, D)
    Qp = np.stack([orc.prepare_query(q, space) for q in Q]).astype(np.float64)
    C64 = C.astype(np.float64)
    S = Qp @ C64.T if space != "l2" else -np.sum((C64[None, :, :] - Qp[:, None, :]) ** 2, axis=2)
    for nprobe in (1, 4, 8, NLIST):
        got = ivf.probe(Q, nprobe)
        assert got.dtype == np.int64 and got.shape == (Q.shape[0], nprobe)
        want = np.argsort(-S, axis=1, kind="stable")[:, :nprobe]
        for j in range(Q.shape[0]):
            assert len(set(got[j].tolist())) == nprobe
            scale = max(1.0, float(np.abs(S[j]).max()))
            for a, b in zip(got[j], want[j]):                           # a differing cell only inside a near tie
                assert a == b or abs(S[j, a] - S[j, b]) <= 1e-5 * scale, (nprobe, j, a, b)


# ------------------------------------------------------------------------------------------------------- 3. full probe
@pytest.mark.parametrize("dim", [64, 96, 50, 768])
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_full_probe_is_the_exact_search(dim, space):
    ivf, exact, Q, _ = _pair(N, dim, space, seed=dim, train_iters=4)
    for eta, pref in ((0.5, 0.0), (0.3, 0.2)):
        singles = [exact.search_batch(Q[j:j + 1], K, eta, pref) for j in range(32)]
        for j in range(6):
            assert _same(ivf.search_batch(Q[j:j + 1], K, eta, pref, nprobe=NLIST), singles[j]), (eta, j)
        for b in (9, 32):
            ids, sc = ivf.search_batch(Q[:b], K, eta, pref, nprobe=NLIST)
            for j in range(b):
                assert _same((ids[j:j + 1], sc[j:j + 1]), singles[j]), (eta, b, j)
    # nprobe beyond nlist probes everything as well, and the one-query form returns the exact (doc id, score, payload) tuples
    got = ivf.search(Q[0], K, 0.5, nprobe=10 * NLIST)
    want = exact.search(Q[0], K, 0.5)
    assert [(r[0], np.float32(r[1]).view(np.uint32)) for r in got] == [(r[0], np.float32(r[1]).view(np.uint32)) for r in want]


# ------------------------------------------------------------------------------------------------------- 4. partial probe
@pytest.mark.parametrize("dim,space", [(64, "cosine"), (64, "l2"), (96, "cosine"), (50, "cosine"), (129, "l2"), (768, "cosine")])
def test_partial_probe_is_the_filtered_search(dim, space):
    ivf, exact, Q, _ = _pair(N, dim, space, seed=dim + 1, train_iters=4)
    for nprobe in (1, 4, 8):
        cells = ivf.probe(Q[:32], nprobe)
        assert len({tuple(sorted(row)) for row in cells.tolist()}) > 4         # the queries probe different cells
        want = [exact.search_batch(Q[j:j + 1], K, 0.4, 0.0, filter=_mask_of(ivf, cells[j])) for j in range(32)]
        for j in range(5):
            assert _same(ivf.search_batch(Q[j:j + 1], K, 0.4, 0.0, nprobe=nprobe), want[j]), (nprobe, j)
        for b in (9, 32):
            ids, sc = ivf.search_batch(Q[:b], K, 0.4, 0.0, nprobe=nprobe)
            assert ids.shape == (b, K) and ids.min() >= 0
            for j in range(b):
                assert _same((ids[j:j + 1], sc[j:j + 1]), want[j]), (nprobe, b, j)
    # the ANN re-rank rule (candidates = k) with a similarity transform
    cells = ivf.probe(Q[:9], 4)
    ids, sc = ivf.search_batch(Q[:9], K, 0.4, 0.1, candidates=K, similarity="one_minus_dist", nprobe=4)
    for j in range(9):
        w = exact.search_batch(Q[j:j + 1], K, 0.4, 0.1, candidates=K, similarity="one_minus_dist", filter=_mask_of(ivf, cells[j]))
        assert _same((ids[j:j + 1], sc[j:j + 1]), w), j
    # the default nprobe (nlist // 64 = 1) and the constructor's
    assert _same(ivf.search_batch(Q[:3], K, 0.4), ivf.search_batch(Q[:3], K, 0.4, nprobe=1))


# ------------------------------------------------------------------------------------------------------- 5. oracle
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_oracle_on_the_probed_rows(space):
    ivf, _, Q, cols = _pair(space=space, seed=5)
    E = ivf._embeddings
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    total = dec = 0
    for nprobe, eta, pref in ((1, 0.3, 0.0), (4, 0.5, 0.2), (8, 0.0, 0.0)):
        cells = ivf.probe(Q[:32], nprobe)
        ids, sc = ivf.search_batch(Q[:32], K, eta, pref, nprobe=nprobe)
        for j in range(32):
            rows = np.nonzero(_mask_of(ivf, cells[j]))[0]
            pos = np.searchsorted(rows, ids[j])
            assert np.all(pos < rows.size) and np.array_equal(rows[np.minimum(pos, rows.size - 1)], ids[j]), "an id outside the probe"
            decisive, msg = compare_query(E[rows], Q[j], dewi32[rows], ent32[rows], K, eta, pref, space, pos, sc[j])
            assert msg is None, f"nprobe {nprobe}, query {j}: {msg}"
            dec += int(decisive)
            total += 1
    assert dec >= default_floor(K) * total, f"only {dec}/{total} decisive queries"


# ------------------------------------------------------------------------------------------------------- 6. recall
def test_recall_at_10():
    """A cap against a broken quantiser: a NumPy model of the training (random-row init, 10 rounds of spherical k-means) gives
    recall@10 = 1.00 on this generator at nprobe 4 and 8 for seeds 0-3; 0.05 is the room for a different initial draw."""
    ivf, exact, Q, _ = _pair(seed=0)
    want, _ = exact.search_batch(Q, K, 0.0)
    got, _ = ivf.search_batch(Q, K, 0.0, nprobe=8)
    recall = float(np.mean([len(set(got[j].tolist()) & set(want[j].tolist())) / K for j in range(Q.shape[0])]))
    print(f"recall@10 at nprobe 8 of 64: {recall:.4f}")
    assert recall >= 0.95, recall


# ------------------------------------------------------------------------------------------------------- 7. short probes
def test_short_and_empty_probes():
    ivf, exact, Q, _ = _pair(600, D, "cosine", seed=2, nlist=512)
    sizes = ivf.cell_sizes
    assert sizes.sum() == 600 and sizes.shape == (512,)
    cells = ivf.probe(Q[:12], 1)
    ids, sc = ivf.search_batch(Q[:12], K, 0.4, nprobe=1)
    assert ids.shape == (12, K) and sc.shape == (12, K)
    n_short = 0
    for j in range(12):
        f = int(sizes[cells[j, 0]])
        kk = min(K, f)
        n_short += int(f < K)
        assert np.all(ids[j, :kk] >= 0) and np.all(ids[j, kk:] == -1) and np.all(np.isnan(sc[j, kk:]))
        if kk:
            assert _same((ids[j:j + 1, :kk], sc[j:j + 1, :kk]), exact.search_batch(Q[j:j + 1], kk, 0.4, filter=_mask_of(ivf, cells[j])))
        res = ivf.search(Q[j], K, 0.4, nprobe=1)
        assert [int(r[0][4:]) for r in res] == ids[j, :kk].tolist()
    assert n_short > 0                                                           # 600 rows in 512 cells: most cells hold 1-2 rows
    # a mixed batch: probes that reach the cut of 2k = 20 rows and probes that do not, together
    mixed = [p for p in range(8, 48)
             if len({bool(_mask_of(ivf, row).sum() >= 2 * K) for row in ivf.probe(Q[:12], p)}) == 2]
    assert mixed, "no nprobe gives long and short probes in one batch"
    cells = ivf.probe(Q[:12], mixed[0])
    ids, sc = ivf.search_batch(Q[:12], K, 0.4, nprobe=mixed[0])
    for j in range(12):
        m = _mask_of(ivf, cells[j])
        kk = min(K, int(m.sum()))
        assert np.all(ids[j, kk:] == -1)
        assert _same((ids[j:j + 1, :kk], sc[j:j + 1, :kk]), exact.search_batch(Q[j:j + 1], kk, 0.4, filter=m)), j


def test_empty_cells_are_searchable():
    ivf, exact, Q, _ = _pair(seed=1, noise=0.35)
    sizes = ivf.cell_sizes
    empty = np.nonzero(sizes == 0)[0]
    assert empty.size > 0, "this generator leaves empty cells"
    q = ivf.centroids[empty[:1]]                                                 # the empty cell's own centroid: it is probed first
    for nprobe in (1, 4):
        cells = ivf.probe(q, nprobe)
        assert np.any(sizes[cells[0]] == 0)
        m = _mask_of(ivf, cells[0])
        res = ivf.search(q[0], K, 0.4, nprobe=nprobe)
        ids, sc = ivf.search_batch(q, K, 0.4, nprobe=nprobe)
        if m.sum() == 0:
            assert res == [] and np.all(ids == -1) and np.all(np.isnan(sc))
        else:
            kk = min(K, int(m.sum()))
            assert _same((ids[:, :kk], sc[:, :kk]), exact.search_batch(q, kk, 0.4, filter=m))
    ids, _ = ivf.search_batch(np.concatenate([q, Q[:8]]), K, 0.4, nprobe=2)      # ... and inside a group
    assert ids.shape == (9, K) and np.all(ids[1:] >= 0)


# ------------------------------------------------------------------------------------------------------- 8. the index
def test_training_is_deterministic_and_persistent(tmp_path):
    from dewi.backends import ExactIndex
    from dewi.ivf import IVFIndex
    ivf, exact, Q, cols = _pair(seed=3, nprobe=4)
    again, _, _, _ = _pair(seed=3, nprobe=4)
    assert np.array_equal(ivf.cell_of_row, again.cell_of_row) and np.array_equal(ivf.centroids, again.centroids)
    other, _, _, _ = _pair(seed=3, nprobe=4, train_seed=1)
    assert not np.array_equal(ivf.cell_of_row, other.cell_of_row)
    want = ivf.search_batch(Q[:9], K, 0.4)
    assert _same(want, ivf.search_batch(Q[:9], K, 0.4, nprobe=4))                # the constructor's nprobe is the default

    ivf.save(tmp_path / "ivf")
    exact.save(tmp_path / "exact")
    assert (tmp_path / "ivf" / "metadata.json").read_bytes() == (tmp_path / "exact" / "metadata.json").read_bytes()
    assert (tmp_path / "ivf" / "payloads.jsonl").read_bytes() == (tmp_path / "exact" / "payloads.jsonl").read_bytes()
    assert {p.name for p in (tmp_path / "ivf").iterdir()} == {"metadata.json", "payloads.jsonl", "embeddings.npy", "ivf.json",
                                                               "ivf_centroids.npy", "ivf_assign.npy"}
    loaded = IVFIndex.load(tmp_path / "ivf")
    loaded._train = None                                                         # load() must not retrain
    assert loaded.nprobe == 4 and loaded.nlist == NLIST
    assert _same(loaded.search_batch(Q[:9], K, 0.4), want)
    assert np.array_equal(loaded.cell_of_row, ivf.cell_of_row) and np.array_equal(loaded.centroids, ivf.centroids)
    as_exact = ExactIndex.load(tmp_path / "ivf")                                 # the same directory is an ExactIndex
    assert type(as_exact) is ExactIndex
    assert _same(as_exact.search_batch(Q[:9], K, 0.4), exact.search_batch(Q[:9], K, 0.4))

    # add + build retrains on all rows
    X2, _ = _clustered(500, D, seed=9)
    ivf.add_batch_columns([f"new_{i}" for i in range(500)], X2, orc.synth_payload_columns(500, seed=9))
    ivf.build()
    assert ivf.cell_of_row.shape == (N + 500,) and ivf.cell_sizes.sum() == N + 500
    exact.add_batch_columns([f"new_{i}" for i in range(500)], X2, orc.synth_payload_columns(500, seed=9))
    assert _same(ivf.search_batch(Q[:3], K, 0.4, nprobe=NLIST), exact.search_batch(Q[:3], K, 0.4))


def test_ivf_errors():
    from dewi.ivf import IVFIndex
    ivf, exact, Q, _ = _pair(2000, D, seed=4, nlist=16)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            ivf.search_batch(Q[:2], K, nprobe=bad)
        with pytest.raises(ValueError):
            ivf.search(Q[0], K, nprobe=bad)
    with pytest.raises(ValueError):
        ivf.search_batch(Q[:2], K, similarity="one_minus_dist")                  # a transform needs candidates=
    with pytest.raises(ValueError):
        ivf.search_batch(Q[:2], K, candidates=K - 1)
    assert ivf.search_batch(Q[:2], 0)[0].shape == (2, 0)
    # a user filter runs the parent's exact filtered search
    mask = np.arange(2000) % 3 == 0
    assert _same(ivf.search_batch(Q[:4], K, 0.4, filter=mask, nprobe=1), exact.search_batch(Q[:4], K, 0.4, filter=mask))
    with pytest.raises(ValueError):
        few = IVFIndex(D, nlist=64)
        X, _ = _clustered(32, D, seed=1, n_queries=4)
        few.add_batch_columns([str(i) for i in range(32)], X, orc.synth_payload_columns(32, seed=1))
        few.build()                                                              # more cells than rows
    ivf._corpus = ivf._corpus.to_bf16()                                          # a bf16 corpus is not served
    with pytest.raises(NotImplementedError):
        ivf.search_batch(Q[:2], K, nprobe=2)


# ------------------------------------------------------------------------------------------------------- 9. full size
def test_ivf_full_size():
    from dewi.backends import ExactIndex
    from dewi.ivf import IVFIndex
    n, dim, nlist, nprobe = 1 << 20, 768, 1024, 16
    r = np.random.RandomState(11)
    cen = r.randn(1024, dim).astype(np.float32)
    X = np.empty((n, dim), np.float32)
    for s in range(0, n, 1 << 16):
        X[s:s + (1 << 16)] = _unit(cen[r.randint(0, 1024, 1 << 16)] + r.randn(1 << 16, dim).astype(np.float32))
    Q = _unit(X[r.choice(n, 32, replace=False)] + 0.05 * r.randn(32, dim).astype(np.float32))
    cols = orc.synth_payload_columns(n, seed=11)
    ids = [f"doc_{i:07d}" for i in range(n)]
    ivf = IVFIndex(dim, nlist=nlist, nprobe=nprobe, train_iters=4)
    ivf.add_batch_columns(ids, X, cols)
    ivf.build()
    sizes = ivf.cell_sizes
    assert sizes.sum() == n
    cells = ivf.probe(Q, nprobe)
    got_ids, got_sc = ivf.search_batch(Q, K, 0.3)
    one = ivf.search_batch(Q[:1], K, 0.3)
    assert _same(one, (got_ids[:1], got_sc[:1]))
    exact = ExactIndex(dim)
    exact._corpus, exact._doc_ids, exact._is_trained = ivf._corpus, ivf._doc_ids, True      # the same device matrix
    for j in range(32):
        want = exact._corpus.search(Q[j:j + 1], K, 0.3, 0.0, filter=exact._corpus.make_filter(_mask_of(ivf, cells[j])))
        assert _same((got_ids[j:j + 1], got_sc[j:j + 1]), want), j


# ------------------------------------------------------------------------------------------------------- 10. > 1024 segments
# nlist * G = 3000, 1200 and 8192 (cell, bucket) segments: the plan's scan takes 3, 2 and 8 rounds of 1024 (csrc/ivf.hip)
MANY_CELLS = [(6000, 50, 1500, "cosine"), (6000, 129, 300, "l2"), (9000, 64, 2048, "cosine")]
MANY_NPROBE = (4, 16, 64)
_many_cells = {}


def _many_cells_pair(n, dim, nlist, space):
    """Built once per shape: -> (ivf, exact, queries)."""
    key = (n, dim, nlist, space)
    if key not in _many_cells:
        _many_cells[key] = _pair(n, dim, space, seed=dim + 1, nlist=nlist, train_iters=4)[:3]
    return _many_cells[key]


def _probe_sizes(ivf, cells):
    """|F_j| of every query (the probed cells of one query are distinct)."""
    return ivf.cell_sizes[cells].sum(axis=1)


@pytest.mark.parametrize("n,dim,nlist,space", MANY_CELLS)
def test_more_than_1024_segments(n, dim, nlist, space):
    ivf, exact, Q = _many_cells_pair(n, dim, nlist, space)
    offsets, _, g = ivf.cell_lists()
    assert nlist * g > 1024 and offsets.shape == (nlist * g + 1,) and offsets[-1] == n
    for nprobe in MANY_NPROBE:
        cells = ivf.probe(Q[:32], nprobe)
        f = _probe_sizes(ivf, cells)
        assert np.array_equal(f, [_mask_of(ivf, row).sum() for row in cells])
        print(f"{n} x {dim}, nlist {nlist}, nprobe {nprobe}: |F_j| {f.min()} to {f.max()}, {int((f < 2 * K).sum())} short probes of 32")
        assert f.min() > 0
        kk = np.minimum(K, f)
        want = [exact.search_batch(Q[j:j + 1], int(kk[j]), 0.4, 0.0, filter=_mask_of(ivf, cells[j])) for j in range(32)]
        got = [ivf.search_batch(Q[j:j + 1], K, 0.4, 0.0, nprobe=nprobe) for j in range(4)]
        where = list(range(4))
        for b in (9, 32):
            ids, sc = ivf.search_batch(Q[:b], K, 0.4, 0.0, nprobe=nprobe)
            got += [(ids[j:j + 1], sc[j:j + 1]) for j in range(b)]
            where += list(range(b))
        for (ids, sc), j in zip(got, where):
            assert ids.shape == (1, K) and np.all(ids[0, kk[j]:] == -1) and np.all(np.isnan(sc[0, kk[j]:])), (nprobe, j)
            assert _same((ids[:, :kk[j]], sc[:, :kk[j]]), want[j]), (nprobe, j)
    # the full probe is the unfiltered exact search
    singles = [exact.search_batch(Q[j:j + 1], K, 0.4, 0.0) for j in range(32)]
    assert _same(ivf.search_batch(Q[:1], K, 0.4, 0.0, nprobe=nlist), singles[0])
    for b in (9, 32):
        ids, sc = ivf.search_batch(Q[:b], K, 0.4, 0.0, nprobe=nlist)
        for j in range(b):
            assert _same((ids[j:j + 1], sc[j:j + 1]), singles[j]), (b, j)


def test_more_than_1024_segments_mix_short_and_long_probes():
    """The cases above take both ways through ``search_device``: some batch of 32 mixes probes below and above the cut of 2k
    rows (the split), some batch is all long (the shared passes alone)."""
    short = {}
    for shape in MANY_CELLS:
        ivf, _, Q = _many_cells_pair(*shape)
        for nprobe in MANY_NPROBE:
            short[shape + (nprobe,)] = int((_probe_sizes(ivf, ivf.probe(Q[:32], nprobe)) < 2 * K).sum())
    assert any(0 < s < 32 for s in short.values()), short
    assert any(s == 0 for s in short.values()), short


# ------------------------------------------------------------------------------------------------------- 11. ties across segments
def _reload_with_assignment(ivf, path, assign):
    """Save, overwrite the saved assignment, load: ``load()`` takes the saved assignment as it is."""
    from dewi.ivf import IVFIndex
    ivf.save(path)
    np.save(str(path / "ivf_assign.npy"), np.asarray(assign, dtype=np.int32))
    return IVFIndex.load(path)


@pytest.mark.parametrize("dim", [64, 50])
def test_exact_ties_across_segments(dim, tmp_path):
    """200 bit-identical copies of each of 100 vectors, scattered over 64 cells by a random assignment: a query's probe holds
    about 50 copies of its vector in several segments of the list, all with one similarity, and the cut of c = 2k = 20 rows
    falls inside them.  Ties on similarity go to the lower row (include/dewi_hip.h), wherever the row sits in the list."""
    from dewi.backends import ExactIndex
    from dewi.ivf import IVFIndex
    n, n_base, nlist, nprobe = 20000, 100, 64, 16
    r = np.random.RandomState(dim)
    B = _unit(r.randn(n_base, dim))
    X = B[np.arange(n) % n_base]
    which = r.choice(n_base, 32, replace=False)
    Q = _unit(B[which] + 0.05 * r.randn(32, dim))
    cols = orc.synth_payload_columns(n, seed=dim)
    ids = [f"doc_{i:07d}" for i in range(n)]
    first = IVFIndex(dim, "cosine", nlist=nlist, train_iters=1)
    first.add_batch_columns(ids, X, cols)
    first.build()
    assign = np.random.RandomState(0).randint(0, nlist, n).astype(np.int32)
    ivf = _reload_with_assignment(first, tmp_path / "ivf", assign)
    exact = ExactIndex(dim, "cosine")
    exact.add_batch_columns(ids, X, cols)
    exact.build()
    E = exact._embeddings
    assert np.array_equal(E[:n_base].view(np.uint32), E[n_base:2 * n_base].view(np.uint32))         # the stored copies are bit-equal

    cells = ivf.probe(Q, nprobe)
    assert np.array_equal(ivf.cell_of_row, assign)
    lowest = []
    for j in range(32):
        copies = np.arange(which[j], n, n_base)
        mine = copies[np.isin(assign[copies], cells[j])]                         # the copies of B[j] inside F_j, ascending
        assert mine.size >= 2 * K + 1 and np.unique(assign[mine]).size >= 2, (j, mine.size)
        lowest.append(mine[:2 * K])
    want = [exact.search_batch(Q[j:j + 1], K, 0.4, 0.1, filter=_mask_of(ivf, cells[j])) for j in range(32)]
    got = [ivf.search_batch(Q[j:j + 1], K, 0.4, 0.1, nprobe=nprobe) for j in range(32)]
    for b in (9, 32):
        ids_b, sc_b = ivf.search_batch(Q[:b], K, 0.4, 0.1, nprobe=nprobe)
        got += [(ids_b[j:j + 1], sc_b[j:j + 1]) for j in range(b)]
    for t, res in enumerate(got):
        j = t if t < 32 else (t - 32 if t < 41 else t - 41)
        assert _same(res, want[j]), (t, j)                                       # 1. the exact search on the mask of F_j
        if dim == 64:
            assert np.all(np.isin(res[0][0], lowest[j])), (t, j, res[0][0], lowest[j])   # 2. the cut took the 20 lowest copies
    if dim == 64:
        for j in range(32):
            assert np.all(np.isin(want[j][0][0], lowest[j])), j


def test_saved_assignment_outside_the_range_is_refused(tmp_path):
    ivf, _, Q, _ = _pair(2000, D, seed=6, nlist=16, train_iters=1)
    assign = ivf.cell_of_row.copy()
    assign[[17, 1999]] = [-1, 16]
    loaded = _reload_with_assignment(ivf, tmp_path / "ivf", assign)
    with pytest.raises(ValueError, match=r"2 rows are assigned to cells outside \[0, 16\)"):
        loaded.search_batch(Q[:2], K, 0.4, nprobe=2)

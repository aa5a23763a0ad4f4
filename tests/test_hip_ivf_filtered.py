"""GPU tests of ``IVFIndex.search_probe_filtered*``: the IVF probe under a user filter.

Contract: query j's answer is, bit for bit, ``ExactIndex.search_batch(q_j, k', ..., filter=<rows of its probed cells> &
<its allow-list>)`` with k' = min(k, |F_j|), the rest of the row id -1 / score NaN; with ``approx=True`` it is
``search_approx_filtered_device`` on the same rows; with ``widen=True`` the same at the smallest doubling of ``nprobe`` at which
|F_j| reaches the cut (or at ``nlist``).  The cells of a query come from ``ivf.probe`` and ``cell_of_row``, as in
tests/test_hip_ivf.py.  Every comparison is exact equality of ids and of score bits.
"""
import numpy as np
import pytest

import wsguard as wsg
from test_hip_ivf import _mask_of, _pair, _same

pytestmark = pytest.mark.gpu

N, NLIST, K = 5000, 16, 5
ETA, PREF = 0.4, 0.1
_built = {}


def _indexes(dim, space, **kw):
    """(IVFIndex, ExactIndex, queries), built once per shape."""
    key = (dim, space, tuple(sorted(kw.items())))
    if key not in _built:
        _built[key] = _pair(N, dim, space, seed=dim, nlist=NLIST, train_iters=3, **kw)[:3]
    return _built[key]


def _user_mask(p, seed=0):
    return np.random.RandomState(seed).rand(N) < p


def _expected(ivf, exact, Q, masks, nprobe, k=K, eta=ETA, pref=PREF, **kw):
    """The contract, query by query: ``masks`` is one bool [N] for everyone or [B, N]; ``nprobe`` an int or one per query."""
    b = Q.shape[0]
    steps = np.broadcast_to(np.asarray(nprobe, np.int64), (b,))
    cells = {int(p): ivf.probe(Q, int(p)) for p in np.unique(steps)}              # the coarse step of the WHOLE batch
    ids = np.full((b, k), -1, np.int64)
    sc = np.full((b, k), np.nan, np.float32)
    sizes = np.zeros(b, np.int64)
    for j in range(b):
        m = _mask_of(ivf, cells[int(steps[j])][j]) & (masks if masks.ndim == 1 else masks[j])
        sizes[j] = m.sum()
        kk = min(k, int(sizes[j]))
        if kk:
            got = exact.search_batch(Q[j:j + 1], kk, eta, pref, filter=m, **kw)
            ids[j, :kk], sc[j, :kk] = got[0][0], got[1][0]
    return (ids, sc), sizes


# ------------------------------------------------------------------------------------------------------- 1. the contract
@pytest.mark.parametrize("dim", [32, 50, 129])
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_every_query_is_the_filtered_search_on_its_cells(dim, space):
    ivf, exact, Q = _indexes(dim, space)
    mask = _user_mask(0.3, seed=dim)
    for b in (1, 3, 32):
        for nprobe in (1, 4):
            want, _ = _expected(ivf, exact, Q[:b], mask, nprobe)
            got = ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=mask, nprobe=nprobe)
            assert got[0].shape == (b, K) and got[0].dtype == np.int64 and got[1].dtype == np.float32
            assert _same(got, want), (b, nprobe)
            assert mask[got[0]].all()
    # the ANN re-rank rule (candidates = k) with a similarity transform
    sim = "one_minus_dist" if space == "cosine" else "inv_one_plus_dist"
    want, _ = _expected(ivf, exact, Q[:9], mask, 4, candidates=K, similarity=sim)
    assert _same(ivf.search_probe_filtered_batch(Q[:9], K, ETA, PREF, K, sim, filter=mask, nprobe=4), want)
    # one query through the SearchResult form
    res = ivf.search_probe_filtered(Q[0], K, ETA, PREF, filter=mask, nprobe=4)
    one = exact.search(Q[0], K, ETA, PREF, filter=_mask_of(ivf, ivf.probe(Q[:1], 4)[0]) & mask)
    assert [(r[0], np.float32(r[1]).view(np.uint32)) for r in res] == [(r[0], np.float32(r[1]).view(np.uint32)) for r in one]


def test_every_form_of_a_filter():
    ivf, exact, Q = _indexes(50, "cosine")
    b, nprobe = 11, 3
    mask = _user_mask(0.3, seed=1)
    want, _ = _expected(ivf, exact, Q[:b], mask, nprobe)
    rows = np.nonzero(mask)[0]
    forms = {"mask": mask, "DeviceFilter": ivf.make_filter(mask), "rows": rows,
             "doc_ids": [f"doc_{i:07d}" for i in rows]}
    for name, f in forms.items():
        assert _same(ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=f, nprobe=nprobe), want), name
    prepared = forms["DeviceFilter"]
    assert prepared._mask is not None and prepared.byte_mask() is prepared._mask         # built once, kept
    assert np.array_equal(prepared.byte_mask().cpu().numpy().astype(bool), mask)
    # dedup_filter: a DeviceFilter like any other
    dedup = ivf.dedup_filter(0.7)
    dmask = dedup.byte_mask().cpu().numpy().astype(bool)
    assert 0 < dmask.sum() == len(dedup) < N
    want_d, _ = _expected(ivf, exact, Q[:b], dmask, nprobe)
    assert _same(ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=dedup, nprobe=nprobe), want_d)
    # per query: a bool [B, N] mask and prepared DeviceQueryFilters
    rs = np.random.RandomState(2)
    per = rs.rand(b, N) < rs.choice([0.1, 0.3, 0.9], b)[:, None]
    want_q, _ = _expected(ivf, exact, Q[:b], per, nprobe)
    assert _same(ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=per, nprobe=nprobe), want_q)
    assert _same(ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=ivf.make_query_filters(per), nprobe=nprobe), want_q)
    assert not _same(want_q, want)
    with pytest.raises(ValueError):
        ivf.search_probe_filtered_batch(Q[:b - 1], K, filter=per, nprobe=nprobe)           # B lists for B - 1 queries


def test_trivial_filters_are_the_known_searches():
    ivf, exact, Q = _indexes(129, "l2")
    mask = _user_mask(0.3, seed=3)
    for b in (1, 11):
        everything = np.ones(N, bool)
        for nprobe in (2, 5):
            assert _same(ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=everything, nprobe=nprobe),
                         ivf.search_batch(Q[:b], K, ETA, PREF, nprobe=nprobe)), (b, nprobe)
        got = ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=mask, nprobe=NLIST)
        for j in range(b):
            assert _same((got[0][j:j + 1], got[1][j:j + 1]), exact.search_batch(Q[j:j + 1], K, ETA, PREF, filter=mask)), (b, j)
    # the existing entry points are untouched: a filter there is the parent's exact search, whatever nprobe says
    assert _same(ivf.search_batch(Q[:4], K, ETA, filter=mask, nprobe=1), exact.search_batch(Q[:4], K, ETA, filter=mask))
    assert ivf.search_probe_filtered_batch(Q[:3], 0, filter=mask)[0].shape == (3, 0)


# ------------------------------------------------------------------------------------------------------- 2. short lists, widening
def _planted(ivf, Q, n_a, n_b):
    """A mask of n_a + n_b rows (about 0.2 % of the corpus): n_a rows of the cell query 0 probes first, n_b rows of the first
    cell of a query that starts elsewhere.  At nprobe 1 the queries of the first cell hold n_a rows, those of the second n_b,
    everyone else none."""
    first = ivf.probe(Q, 1)[:, 0]
    assert len(set(first.tolist())) >= 3, "the queries start in at least three cells"
    cell_a = int(first[0])
    cell_b = int(first[first != cell_a][0])
    cells = ivf.cell_of_row
    rows_a, rows_b = np.nonzero(cells == cell_a)[0], np.nonzero(cells == cell_b)[0]
    assert rows_a.size >= n_a and rows_b.size >= n_b
    mask = np.zeros(N, bool)
    mask[rows_a[:: rows_a.size // n_a][:n_a]] = True
    mask[rows_b[:n_b]] = True
    assert mask.sum() == n_a + n_b
    return mask


def _sparse_case():
    ivf, exact, Q = _indexes(32, "cosine")
    return ivf, exact, Q[:32], _planted(ivf, Q[:32], 2 * K, 2)       # 12 rows of 5000: 0.24 %


def test_short_and_empty_lists():
    ivf, exact, Q, mask = _sparse_case()
    for nprobe in (1, 4):
        want, sizes = _expected(ivf, exact, Q, mask, nprobe)
        if nprobe == 1:
            assert (sizes == 0).any() and ((sizes > 0) & (sizes < K)).any(), sizes
        got = ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=mask, nprobe=nprobe)
        assert _same(got, want), nprobe
        for j in range(Q.shape[0]):
            kk = min(K, int(sizes[j]))
            assert np.all(got[0][j, :kk] >= 0) and np.all(got[0][j, kk:] == -1) and np.all(np.isnan(got[1][j, kk:]))
        one = ivf.search_probe_filtered(Q[int(np.argmin(sizes))], K, ETA, PREF, filter=mask, nprobe=nprobe)
        assert len(one) == min(K, int(sizes.min()))
    # lists below the cut 2k but not below k, next to long and empty ones
    mid = _planted(ivf, Q, K + 2, 6 * K)
    want, sizes = _expected(ivf, exact, Q, mid, 1)
    assert ((sizes >= K) & (sizes < 2 * K)).any() and (sizes >= 2 * K).any() and (sizes == 0).any(), sizes
    assert _same(ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=mid, nprobe=1), want)


def _widen_model(ivf, Q, masks, nprobe, cut):
    """nprobe_j: doubled from ``nprobe`` (capped at nlist) until the allowed rows of query j's cells reach the cut."""
    b = Q.shape[0]
    used = np.zeros(b, np.int64)
    p, todo = nprobe, list(range(b))
    while todo:
        cells = ivf.probe(Q, p)
        size = lambda j: int((_mask_of(ivf, cells[j]) & (masks if masks.ndim == 1 else masks[j])).sum())
        again = [j for j in todo if size(j) < cut and p < NLIST]
        for j in todo:
            used[j] = p
        todo, p = again, min(2 * p, NLIST)
    return used


@pytest.mark.parametrize("per_query", [False, True])
def test_widen(per_query):
    ivf, exact, Q, mask = _sparse_case()
    if per_query:
        masks = np.stack([mask if j % 3 else _user_mask(0.3, seed=10 + j) for j in range(Q.shape[0])])
    else:
        masks = mask
    used = _widen_model(ivf, Q, masks, 1, 2 * K)
    assert (used == 1).any() and (used > 1).any(), used              # somebody widens, somebody does not
    want, sizes = _expected(ivf, exact, Q, masks, used)
    assert np.all((sizes >= 2 * K) | (used == NLIST))
    ids, sc, got_used = ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=masks, nprobe=1, widen=True, return_nprobe=True)
    assert got_used.dtype == np.int64 and got_used.tolist() == used.tolist()
    assert _same((ids, sc), want)
    # widen=False: one probe, a constant nprobe_used
    ids, sc, flat = ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=masks, nprobe=2, return_nprobe=True)
    assert flat.tolist() == [2] * Q.shape[0]
    assert _same((ids, sc), _expected(ivf, exact, Q, masks, 2)[0])
    # a mask that holds fewer rows than the cut widens everyone to nlist: the exact filtered search (3 queries keep it quick)
    if not per_query:
        few = _planted(ivf, Q, K, 2)
        ids, sc, top = ivf.search_probe_filtered_batch(Q[:3], K, ETA, PREF, filter=few, nprobe=1, widen=True, return_nprobe=True)
        assert top.tolist() == [NLIST] * 3 and few.sum() == K + 2 < 2 * K
        for j in range(3):
            assert _same((ids[j:j + 1], sc[j:j + 1]), exact.search_batch(Q[j:j + 1], K, ETA, PREF, filter=few))
        res, p = ivf.search_probe_filtered(Q[0], K, ETA, PREF, filter=few, nprobe=1, widen=True, return_nprobe=True)
        assert p == NLIST and len(res) == K


# ------------------------------------------------------------------------------------------------------- 3. int8 codes
@pytest.mark.parametrize("dim", [32, 64])
@pytest.mark.parametrize("rescore", [True, False])
def test_approx_is_the_int8_filtered_search_on_the_same_rows(dim, rescore):
    import torch
    ivf, _, Q = _indexes(dim, "cosine", int8_codes=True)
    corpus = ivf._corpus
    Q = Q[:11]
    Q_dev = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    for mask, nprobe in ((_user_mask(0.3, seed=dim), 3), (_planted(ivf, Q, 6 * K, 3), 1)):
        cells = ivf.probe(Q, nprobe)
        got = ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=mask, nprobe=nprobe, approx=True, rescore=rescore)
        n_short = n_long = 0
        for j in range(Q.shape[0]):
            m = _mask_of(ivf, cells[j]) & mask
            kk = min(K, int(m.sum()))
            n_short += int(m.sum() < 2 * K)
            n_long += int(m.sum() >= 2 * K)
            assert np.all(got[0][j, kk:] == -1) and np.all(np.isnan(got[1][j, kk:]))
            if kk:
                ids_d, sc_d = corpus.search_approx_filtered_device(Q_dev[j:j + 1], kk, ETA, PREF, corpus.make_filter(m), None, rescore)
                assert _same((got[0][j:j + 1, :kk], got[1][j:j + 1, :kk]), (ids_d.cpu().numpy(), sc_d.cpu().numpy())), (nprobe, j)
        assert n_long > 0 and (n_short > 0) == (nprobe == 1)           # the planted mask: long, short and empty lists together
    with pytest.raises(ValueError, match="at most 1024"):
        ivf.search_probe_filtered_batch(Q, 10, candidates=1025, filter=mask, approx=True)
    with pytest.raises(ValueError):
        ivf.search_probe_filtered_batch(Q, K, candidates=K, similarity="one_minus_dist", filter=mask, approx=True)


# ------------------------------------------------------------------------------------------------------- 4. stale filters, scratch
def test_stale_filters_raise():
    import dewi_oracle as orc
    from test_hip_ivf import _clustered
    ivf, _, Q, _ = _pair(2000, 32, "cosine", seed=7, nlist=NLIST, train_iters=2)
    mask = np.arange(2000) % 3 == 0
    f = ivf.make_filter(mask)
    qf = ivf.make_query_filters(np.stack([mask, ~mask]))
    assert ivf.search_probe_filtered_batch(Q[:2], K, filter=f, nprobe=2)[0].shape == (2, K)
    assert ivf.search_probe_filtered_batch(Q[:2], K, filter=qf, nprobe=2)[0].shape == (2, K)
    ivf.remove(["doc_0000003", "doc_0000004"])
    for stale in (f, qf):
        with pytest.raises(ValueError):
            ivf.search_probe_filtered_batch(Q[:2], K, filter=stale, nprobe=2)
    f = ivf.make_filter(np.arange(1998) % 3 == 0)
    assert ivf.search_probe_filtered_batch(Q[:2], K, filter=f, nprobe=2)[0].min() >= 0
    X2, _ = _clustered(100, 32, seed=9, n_queries=4)
    ivf.add_batch_columns([f"new_{i}" for i in range(100)], X2, orc.synth_payload_columns(100, seed=9))
    ivf.build()
    with pytest.raises(ValueError):
        ivf.search_probe_filtered_batch(Q[:2], K, filter=f, nprobe=2)
    with pytest.raises(ValueError):
        ivf.search_probe_filtered(Q[0], K, filter=f, nprobe=2)


def test_answers_do_not_depend_on_what_the_scratch_held():
    import torch
    ivf, exact, Q = _indexes(50, "l2")
    b, nprobe = 11, 1
    mask = _planted(ivf, Q[:b], 6 * K, 3)                           # long, short and empty lists: every buffer use of the call
    want, sizes = _expected(ivf, exact, Q[:b], mask, nprobe)
    assert ((sizes > 0) & (sizes < 2 * K)).any() and (sizes >= 2 * K).any() and (sizes == 0).any()
    f = ivf.make_filter(mask)
    q_dev = torch.from_numpy(np.ascontiguousarray(Q[:b])).cuda()
    call = lambda: ivf.search_probe_filtered_device(q_dev, K, ETA, PREF, filter=f, nprobe=nprobe)
    base = call()                                                  # sizes the buffers
    torch.cuda.synchronize()
    assert _same((base[0].cpu().numpy(), base[1].cpu().numpy()), want)
    assert ivf._probe_buf is not None and ivf._ivf_ws is not None
    assert wsg.guard(ivf) == 2
    try:
        for pattern in ("0xff", "random"):
            wsg.poison(ivf, pattern, seed=3)
            got = call()
            torch.cuda.synchronize()
            wsg.check(ivf)
            wsg.assert_bit_equal(got, base, pattern)
    finally:
        wsg.release(ivf)
        ivf._probe_buf = ivf._ivf_ws = None

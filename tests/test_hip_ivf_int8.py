"""GPU, Python layer: IVF probes and allow-lists on the int8 codes (``IVFIndex(int8_codes=True)``,
``ExactIndex.search_approx_filtered``).  Every comparison is bit for bit: the int8 scores are integers, the
re-scoring and the blend are one fixed sequence of fp32 operations per record, so neither the kernel geometry nor the grouping
of a batch can change an answer.  No recall floor: the device's answer is the model's, recall belongs to the benchmark.
"""
import numpy as np
import pytest

import int8_list_model as lm
import int8_model as im
from test_hip_int8 import columns, prepare_dev, same_bits

pytestmark = pytest.mark.gpu

N, NLIST = 4099, 16
_cache = {}


def make(cls, x, cols, ids=None, **kwargs):
    ids = [f"d{i:06d}" for i in range(x.shape[0])] if ids is None else ids
    idx = cls(x.shape[1], **kwargs)
    idx.add_batch_columns(ids, x, cols)
    idx.build()
    return idx


def built(dim):
    """(raw rows, payload columns, queries, IVFIndex with codes) — once per dim."""
    from dewi.ivf import IVFIndex
    if dim not in _cache:
        rs = np.random.RandomState(dim)
        x = rs.randn(N, dim).astype(np.float32)
        x[50:56] = x[49]                                   # exact ties, spread over the cells by the maintenance test below
        cols = columns(N, dim)
        q = rs.randn(11, dim).astype(np.float32)
        q[1] = x[49]
        _cache[dim] = (x, cols, q, make(IVFIndex, x, cols, nlist=NLIST, train_iters=2, int8_codes=True))
    return _cache[dim]


def probe_masks(idx, q, nprobe):
    cells, pr = idx.cell_of_row, idx.probe(q, nprobe)
    return np.stack([np.isin(cells, pr[j]) for j in range(q.shape[0])])


def model_answer(idx, q, masks, k, eta, pref, c=None):
    """The model's int8-scored ranking on the index's CURRENT stored rows: ids [B, k] (-1 padded), scores [B, k] (NaN padded)."""
    import torch
    corpus = idx._corpus
    codes, scales = corpus._int8()
    rc, rsc = codes.cpu().numpy(), scales.cpu().numpy()
    stored_c, stored_s = im.quantize(corpus.emb.cpu().numpy())
    assert np.array_equal(rc, stored_c) and same_bits(rsc, stored_s), "the codes are Q of the current stored rows"
    qc, qs, _ = prepare_dev(torch.from_numpy(q).cuda())
    dewi, ent = corpus.dewi32.cpu().numpy(), corpus.ent32.cpu().numpy()
    ids = np.full((q.shape[0], k), -1, np.int64)
    sc = np.full((q.shape[0], k), np.nan, np.float32)
    for j in range(q.shape[0]):
        n_j = int(masks[j].sum())
        if n_j == 0:
            continue
        cj, kj = min(2 * k if c is None else c, n_j), min(k, n_j)
        recs = lm.candidates_filtered(rc, rsc, qc[j:j + 1], qs[j:j + 1], dewi, ent, cj, masks[j])
        a, b = im.search(recs, kj, eta, pref)
        ids[j, :kj], sc[j, :kj] = a[0], b[0]
    return ids, sc


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("b", [1, 8, 11])
def test_probe_equals_the_filtered_approximate_search_on_its_cells(dim, b):
    import torch
    x, cols, q, idx = built(dim)
    q = q[:b]
    corpus = idx._corpus
    for nprobe, k, cand, eta, pref, rescore in ((3, 10, None, 0.3, 0.2, True), (2, 7, 100, 0.0, 0.0, True), (3, 10, None, 0.3, 0.0, False),
                                                (5, 150, None, 0.3, 0.2, True)):
        rows, scores = idx.search_batch(q, k, eta, pref, cand, approx=True, rescore=rescore, nprobe=nprobe)
        masks = probe_masks(idx, q, nprobe)
        assert (masks.sum(axis=1) >= (2 * k if cand is None else cand)).all()
        Q_dev = torch.from_numpy(q).cuda()
        for j in range(b):
            ids_d, sc_d = corpus.search_approx_filtered_device(Q_dev[j:j + 1], k, eta, pref, corpus.make_filter(masks[j]), cand, rescore)
            assert np.array_equal(rows[j], ids_d.cpu().numpy()[0]), (nprobe, k, j)
            assert same_bits(scores[j], sc_d.cpu().numpy()[0]), (nprobe, k, j)
            assert masks[j][rows[j]].all()
        if not rescore:
            want_ids, want_sc = model_answer(idx, q, masks, k, eta, pref, cand)
            assert np.array_equal(rows, want_ids) and same_bits(scores, want_sc)
        auto = idx.search_batch(q, k, eta, pref, cand, rescore=rescore, nprobe=nprobe)           # None: the index has codes
        if idx.APPROX_AUTO_MAX_BATCH is None or b <= idx.APPROX_AUTO_MAX_BATCH:
            assert np.array_equal(auto[0], rows) and same_bits(auto[1], scores)
    one = idx.search(q[0], 5, 0.3, 0.2, approx=True, nprobe=3)
    rows, scores = idx.search_batch(q[:1], 5, 0.3, 0.2, approx=True, nprobe=3)
    assert [int(r[0][1:]) for r in one] == rows[0].tolist() and same_bits(np.array([r[1] for r in one], np.float32), scores[0])


@pytest.mark.parametrize("dim", [64, 768])
def test_every_cell_probed_equals_the_unfiltered_int8_route(dim):
    from dewi.backends import ExactIndex
    x, cols, q, idx = built(dim)
    exact = make(ExactIndex, x, cols, int8_shadow=True)
    for k, cand, rescore in ((10, None, True), (10, None, False), (5, 300, True), (150, None, True)):
        a = idx.search_batch(q, k, 0.3, 0.2, cand, approx=True, rescore=rescore, nprobe=NLIST)
        b = exact.search_batch(q, k, 0.3, 0.2, cand, approx=True, rescore=rescore)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]), (k, cand, rescore)


@pytest.mark.parametrize("dim", [64, 768])
def test_the_fp32_probe_is_unchanged(dim):
    from dewi.ivf import IVFIndex
    x, cols, q, idx = built(dim)
    plain = make(IVFIndex, x, cols, nlist=NLIST, train_iters=2)
    assert np.array_equal(plain.cell_of_row, idx.cell_of_row)
    for k, cand in ((10, None), (7, 100)):
        a = idx.search_batch(q, k, 0.3, 0.2, cand, approx=False, nprobe=3)
        b = plain.search_batch(q, k, 0.3, 0.2, cand, nprobe=3)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    with pytest.raises(ValueError, match="int8_codes=True"):
        plain.search_batch(q, 10, approx=True)
    with pytest.raises(ValueError, match="at most 1024"):
        idx.search_batch(q, 600, approx=True)
    filtered = idx.search_batch(q, 5, 0.3, 0.0, filter=np.arange(N) % 2 == 0)       # None + filter: the parent's exact search
    assert (filtered[0] % 2 == 0).all()


def test_short_and_empty_probes_are_padded():
    """Cell 3 is emptied and cell 4 cut to 5 rows (the lists rebuilt from the edited cell column): a query that probes only
    the empty cell returns -1 / NaN, one that probes the short cell returns its 5 rows, cut and k limited to 5."""
    import torch
    from dewi.ivf import IVFIndex
    dim = 64
    x, cols, q, _ = built(dim)
    idx = make(IVFIndex, x, cols, nlist=NLIST, train_iters=2, int8_codes=True)
    st = idx._ivf
    assign = st.assign.clone()
    cell4 = torch.nonzero(assign == 4).flatten()
    assert cell4.numel() > 5
    assign[assign == 3] = 0
    assign[cell4[5:]] = 1
    st.assign = assign
    idx._make_lists(st, assign, N)
    cents = idx.centroids
    qq = np.stack([cents[3], cents[4], q[0], cents[4] + 0.01 * q[2]]).astype(np.float32)
    assert idx.probe(qq, 1)[:2, 0].tolist() == [3, 4]
    for rescore in (False, True):
        rows, scores = idx.search_batch(qq, 10, 0.3, 0.2, approx=True, rescore=rescore, nprobe=1)
        masks = probe_masks(idx, qq, 1)
        assert masks.sum(axis=1)[:2].tolist() == [0, 5]
        assert (rows[0] == -1).all() and np.isnan(scores[0]).all()
        assert sorted(rows[1, :5].tolist()) == cell4[:5].cpu().tolist() and (rows[1, 5:] == -1).all() and np.isnan(scores[1, 5:]).all()
        if not rescore:
            want_ids, want_sc = model_answer(idx, qq, masks, 10, 0.3, 0.2)
            assert np.array_equal(rows, want_ids) and same_bits(scores, want_sc)
        else:
            corpus = idx._corpus
            for j in (1, 2, 3):
                kk = min(10, int(masks[j].sum()))
                if kk == 0:
                    continue
                ids_d, sc_d = corpus.search_approx_filtered_device(torch.from_numpy(qq[j:j + 1]).cuda(), kk, 0.3, 0.2,
                                                                   corpus.make_filter(masks[j]))
                assert np.array_equal(rows[j, :kk], ids_d.cpu().numpy()[0]) and same_bits(scores[j, :kk], sc_d.cpu().numpy()[0])
    assert len(idx.search(qq[0], 10, approx=True, nprobe=1)) == 0 and len(idx.search(qq[1], 10, approx=True, nprobe=1)) == 5


def test_mutated_index_answers_on_its_current_rows_and_cells():
    from dewi.ivf import IVFIndex
    dim, n = 64, 1500
    rs = np.random.RandomState(5)
    x = rs.randn(n + 40, dim).astype(np.float32)
    cols = columns(n + 40, 5)
    ids = [f"d{i:06d}" for i in range(n + 40)]
    idx = make(IVFIndex, x[:n], {k: v[:n] for k, v in cols.items()}, ids[:n], nlist=NLIST, train_iters=2, int8_codes=True)
    q = rs.randn(9, dim).astype(np.float32)
    idx.search_batch(q, 10, approx=True, nprobe=3)                        # the codes are in use before the mutation
    idx.remove([ids[i] for i in range(0, 300, 7)])
    assert idx._corpus._i8_stale
    up = list(range(n, n + 40)) + [500, 501, 502]
    new_rows = x[up].copy()
    new_rows[-3:] = rs.randn(3, dim).astype(np.float32)
    from dewi.types import payloads_from_columns
    idx.upsert_batch([ids[i] for i in up], new_rows, payloads_from_columns({k: v[up] for k, v in cols.items()}))
    assert idx._corpus._i8_stale
    for nprobe in (2, NLIST):
        masks = probe_masks(idx, q, nprobe)
        rows, scores = idx.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=False, nprobe=nprobe)
        want_ids, want_sc = model_answer(idx, q, masks, 10, 0.3, 0.2)
        assert np.array_equal(rows, want_ids) and same_bits(scores, want_sc), nprobe
    assert not idx._corpus._i8_stale and idx._corpus.n_rows == n - 43 + 40


def test_save_load_round_trip(tmp_path):
    from dewi.ivf import IVFIndex
    x, cols, q, idx = built(64)
    idx.save(tmp_path / "ix")
    back = IVFIndex.load(tmp_path / "ix", int8_codes=True)
    assert not any(p.name.startswith("int8") or "codes" in p.name for p in (tmp_path / "ix").iterdir())
    for rescore in (False, True):
        a = idx.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=rescore, nprobe=3)
        b = back.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=rescore, nprobe=3)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    assert np.array_equal(back._corpus.i8_codes.cpu().numpy(), idx._corpus.i8_codes.cpu().numpy())
    no_codes = IVFIndex.load(tmp_path / "ix")
    with pytest.raises(ValueError, match="int8_codes=True"):
        no_codes.search_batch(q, 10, approx=True)


# ------------------------------------------------------------------------------------------------------------ ExactIndex
def filter_rows(f):
    """The rows of a prepared one-list filter, read back from its buffer."""
    import torch
    return f.buf.view(torch.int32)[16:16 + f.n_allowed].cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("dim", [64, 768])
def test_exact_index_search_approx_filtered(dim):
    from dewi.backends import ExactIndex
    x, cols, q, _ = built(dim)
    key = ("exact", dim)
    if key not in _cache:
        _cache[key] = make(ExactIndex, x, cols, int8_shadow=True)
    idx = _cache[key]
    k, eta, pref = 10, 0.3, 0.2
    rs = np.random.RandomState(3)
    mask = rs.rand(N) < 0.3
    mask[49:56] = np.arange(7) % 2 == 0                  # the list splits the identical rows
    # a mask, and the same list as a prepared filter
    for rescore in (False, True):
        a = idx.search_approx_filtered_batch(q, k, eta, pref, filter=mask, rescore=rescore)
        b = idx.search_approx_filtered_batch(q, k, eta, pref, filter=idx.make_filter(mask), rescore=rescore)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and mask[a[0]].all()
        if not rescore:
            want = model_answer(idx, q, np.broadcast_to(mask, (q.shape[0], N)), k, eta, pref)
            assert np.array_equal(a[0], want[0]) and same_bits(a[1], want[1])
            assert {49, 51, 53, 55} <= set(a[0][1].tolist())
    # candidates, and the facade's single-query form
    a = idx.search_approx_filtered_batch(q, 5, eta, pref, 300, filter=mask, rescore=False)
    want = model_answer(idx, q, np.broadcast_to(mask, (q.shape[0], N)), 5, eta, pref, 300)
    assert np.array_equal(a[0], want[0]) and same_bits(a[1], want[1])
    one = idx.search_approx_filtered(q[1], 5, eta, pref, 300, filter=mask, rescore=False)
    assert [int(r[0][1:]) for r in one] == want[0][1].tolist()
    # per-query filters: lists of every length class — longer than the cut, shorter than it, empty
    masks = np.stack([rs.rand(N) < p for p in rs.uniform(0.2, 0.6, q.shape[0])])
    masks[2] = False
    masks[3] = False
    masks[3, [5, 900, 4000]] = True
    masks[4] = False
    masks[4, rs.choice(N, 15, replace=False)] = True
    qf = idx.make_query_filters(masks)
    for rescore in (False, True):
        a = idx.search_approx_filtered_batch(q, 3, eta, pref, filter=qf, rescore=rescore)
        assert (a[0][2] == -1).all() and np.isnan(a[1][2]).all()
        for j in range(q.shape[0]):
            if masks[j].any():
                b = idx.search_approx_filtered_batch(q[j:j + 1], 3, eta, pref, filter=masks[j], rescore=rescore)
                assert np.array_equal(a[0][j], b[0][0]) and same_bits(a[1][j], b[1][0]), j
        if not rescore:
            want = model_answer(idx, q, masks, 3, eta, pref)
            assert np.array_equal(a[0], want[0]) and same_bits(a[1], want[1])
    with pytest.raises(ValueError, match="query 3: k = 10 exceeds the 3 rows"):
        idx.search_approx_filtered_batch(q, 10, filter=qf)
    # dedup_filter: a normal prepared filter
    f = idx.dedup_filter(0.95)
    dmask = np.zeros(N, bool)
    dmask[filter_rows(f)] = True
    assert dmask[49:56].sum() == 1 and f.n_allowed == N - 6
    a = idx.search_approx_filtered_batch(q, k, eta, pref, filter=f, rescore=False)
    want = model_answer(idx, q, np.broadcast_to(dmask, (q.shape[0], N)), k, eta, pref)
    assert np.array_equal(a[0], want[0]) and same_bits(a[1], want[1])
    # k above |A|, an empty filter, a stale filter
    few = np.zeros(N, bool)
    few[:4] = True
    with pytest.raises(ValueError, match="k = 10 exceeds the 4 rows"):
        idx.search_approx_filtered_batch(q, 10, filter=few)
    assert idx.search_approx_filtered_batch(q, 10, filter=np.zeros(N, bool))[0].shape == (q.shape[0], 0)
    other = make(ExactIndex, x[:200], {k_: v[:200] for k_, v in cols.items()}, int8_shadow=True)
    with pytest.raises(ValueError, match="prepared for another corpus"):
        idx.search_approx_filtered_batch(q, k, filter=other.make_filter(np.ones(200, bool)))
    # the pinned refusals stay
    with pytest.raises(ValueError, match="does not take a filter"):
        idx.search_batch(q, k, approx=True, filter=mask)
    exact = idx.search_batch(q[:2], k, eta, pref, filter=mask)                       # None + filter: the exact path
    plain = idx.search_batch(q[:2], k, eta, pref, approx=False, filter=mask)
    assert np.array_equal(exact[0], plain[0]) and same_bits(exact[1], plain[1])

"""GPU tests of per-query filters: ``search_batch(Q, k, filter=QF)`` where query j searches only its own allow-list F_j.

Contract: query j's ids and scores are bit-equal to the one-list search ``search(Q[j:j+1], k, filter=make_filter(F_j))``,
whatever the batch around it and however its list overlaps the others.  Lists at least as long as the batch's cut share one
pass of the QMASK row kernels over the union of the lists; shorter ones take the one-list search on their own.  An empty
list pads its row with id -1 / score NaN (``ExactIndex``, ``DeviceCorpus``) or gives ``[]`` (``DewiIndex``).
"""
import numpy as np
import pytest

import dewi_oracle as orc
from parity import compare_query

pytestmark = pytest.mark.gpu

FAST_DIMS = [256, 768, 1536]
ANY_DIMS = [384, 1000, 3072]
SHORT_DIMS = [64, 100]
ODD_DIMS = [5, 50, 129, 301, 1001]
GENERIC_DIMS = [4100, 4101]   # 1025 units per row: the generic kernel with 16-byte loads; 4101: with scalar loads
ALL_DIMS = FAST_DIMS + ANY_DIMS + SHORT_DIMS + ODD_DIMS + GENERIC_DIMS


def _eng():
    from dewi import _engine
    return _engine


def _period(dim):
    """Residue period of an fp32 row's offset inside its 16-byte unit."""
    rb = 4 * dim
    tz = 0
    while tz < 4 and (rb >> tz) % 2 == 0:
        tz += 1
    return 16 >> tz


def _corpus(n, dim, space, seed):
    raw = orc.synth_corpus(n, dim, seed=seed)
    cols = orc.synth_payload_columns(n, seed=seed)
    c = _eng().DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    return c, c.emb.cpu().numpy(), dewi32, ent32


def _nine_masks(n, dim, seed):
    """One list per query of a batch of 9: every kind of list, two equal ones, one disjoint from the rest but "all"."""
    rs = np.random.RandomState(seed)
    g = max(_period(dim), 4)
    m = np.zeros((9, n), bool)
    m[0] = rs.rand(n) < 0.30
    m[1, rs.choice(n, max(n // 100, 12), replace=False)] = True       # ~1 %
    m[2] = (np.arange(n) % g) == 1                                     # one residue class
    m[3, n // 3: n // 3 + n // 5] = True                               # a block
    m[4, :8] = True                                                    # the first and last rows (shorter than 2k)
    m[4, n - 8:] = True
    m[5] = True                                                        # every row
    m[6] = m[0]                                                        # equal to another query's list
    free = np.nonzero(~m[[0, 1, 2, 3, 4]].any(axis=0))[0]
    m[7, rs.choice(free, min(free.size, 60), replace=False)] = True   # disjoint from the others (but "all")
    m[8] = rs.rand(n) < 0.05
    return m


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _check_singles(c, Q, masks, k, eta, pref, **kw):
    """The batch under per-query filters against one one-list search per query: bit-equal, -1 / NaN for empty lists."""
    qf = c.make_query_filters(masks)
    assert qf.n_queries == len(qf) == masks.shape[0]
    assert np.array_equal(qf.n_allowed, masks.sum(axis=1))
    assert qf.n_union == int(masks.any(axis=0).sum())
    ids, sc = c.search(Q, k, eta, pref, filter=qf, **kw)
    assert ids.shape == (Q.shape[0], k) and sc.shape == (Q.shape[0], k)
    for j in range(Q.shape[0]):
        if not masks[j].any():
            assert np.all(ids[j] == -1) and np.all(np.isnan(sc[j])), j
            continue
        want = c.search(Q[j:j + 1], k, eta, pref, filter=c.make_filter(masks[j]), **kw)
        assert _same((ids[j:j + 1], sc[j:j + 1]), want), j
    return ids, sc


# ---------------------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("dim", ALL_DIMS)
def test_query_filters_equal_singles_bits(dim):
    n = 2003 if dim <= 1600 else 1201
    for space in ("cosine", "l2"):
        c, _, _, _ = _corpus(n, dim, space, seed=dim + 51)
        Q = orc.synth_queries(9, dim, seed=dim + 53)
        masks = _nine_masks(n, dim, seed=dim)
        _check_singles(c, Q, masks, 10, 0.3, 0.1)                      # 8 + 1 (fast) or 4 + 4 + 1 passes
        _check_singles(c, Q[:5], masks[[0, 3, 5, 6, 2]], 10, 0.3, 0.0, candidates=30)
        big = [j for j in range(9) if masks[j].sum() >= 300]
        for k in (100, 150):                                           # per-wave lists, dense keys
            _check_singles(c, Q[big], masks[big], k, 0.5, 0.2)


# ---------------------------------------------------------------------------------------------------------------- 2. oracle
@pytest.mark.parametrize("dim", [100, 301, 768, 1000, 4100, 4101])
def test_query_filters_oracle_parity(dim):
    n = 2003 if dim <= 1600 else 1201
    k = 10
    total = dec = 0
    for space in ("cosine", "l2"):
        c, E, dewi32, ent32 = _corpus(n, dim, space, seed=dim + 61)
        Q = orc.synth_queries(9, dim, seed=dim + 63)
        masks = _nine_masks(n, dim, seed=dim + 1)
        ids, sc = c.search(Q, k, 0.3, 0.0, filter=c.make_query_filters(masks))
        for j in range(9):
            rows = np.nonzero(masks[j])[0]
            kk = min(k, rows.size)
            pos = np.searchsorted(rows, ids[j, :kk])
            assert np.all(pos < rows.size) and np.array_equal(rows[np.minimum(pos, rows.size - 1)], ids[j, :kk]), \
                f"query {j}: an id outside its list"
            decisive, msg = compare_query(E[rows], Q[j], dewi32[rows], ent32[rows], kk, 0.3, 0.0, space, pos, sc[j, :kk])
            assert msg is None, f"{space} query {j}: {msg}"
            dec += int(decisive)
            total += 1
    assert dec >= 0.5 * total, f"only {dec}/{total} decisive queries"


# ---------------------------------------------------------------------------------------------------------------- 3. leaks
@pytest.mark.parametrize("dim", [5, 50, 129, 301, 768, 1001])
def test_query_filters_no_leak_between_queries(dim):
    """Row r is an exact copy of the vector that queries a and b share; r is on a's list only.  It must come first for a
    and never appear for b — in one pass (a, b neighbours) and across passes."""
    n = 1601
    rs = np.random.RandomState(dim)
    raw = orc.synth_corpus(n, dim, seed=dim + 71)
    Q = orc.synth_queries(9, dim, seed=dim + 73)
    cols = orc.synth_payload_columns(n, seed=dim)
    for a, b in ((1, 2), (0, 8)):
        r = int(rs.randint(n))
        Qx = Q.copy()
        Qx[a] = Qx[b]
        rawx = raw.copy()
        rawx[r] = Qx[b]
        masks = rs.rand(9, n) < 0.5
        masks[a, r] = True
        masks[b, r] = False
        for space in ("cosine", "l2"):
            c = _eng().DeviceCorpus.from_host(rawx, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space)
            ids, _ = c.search(Qx, 10, 0.0, 0.0, filter=c.make_query_filters(masks))
            assert ids[a, 0] == r, (space, a, b)
            assert r not in ids[b].tolist(), (space, a, b)
            for j in range(9):
                assert masks[j, ids[j]].all(), (space, j)


# ---------------------------------------------------------------------------------------------------------------- 4. many
@pytest.mark.parametrize("dim,b", [(768, 33), (100, 70), (301, 33), (1000, 70)])
def test_query_filters_many_queries(dim, b):
    """More than 32 queries: several words of query bits per row."""
    n = 3001
    rs = np.random.RandomState(dim + b)
    c, _, _, _ = _corpus(n, dim, "cosine", seed=dim + 81)
    Q = orc.synth_queries(b, dim, seed=dim + 83)
    masks = rs.rand(b, n) < rs.uniform(0.05, 0.6, size=(b, 1))
    _check_singles(c, Q, masks, 10, 0.3, 0.0)


# ---------------------------------------------------------------------------------------------------------------- 5. rules
def _index(n=1500, dim=96, space="cosine"):
    from dewi.backends import ExactIndex
    from dewi.types import payloads_from_columns
    raw = orc.synth_corpus(n, dim, seed=5)
    cols = orc.synth_payload_columns(n, seed=5)
    idx = ExactIndex(dim, space)
    idx.add_batch([f"d{i}" for i in range(n)], raw, payloads_from_columns(cols))
    idx.build()
    return idx, raw, cols


def test_query_filters_rules():
    idx, raw, _ = _index()
    n, d = raw.shape
    Q = orc.synth_queries(3, d, seed=9)
    masks = np.zeros((3, n), bool)
    masks[0, ::50] = True                                     # 30 rows
    masks[1, 1::3] = True                                     # 500 rows
    qf = idx.make_query_filters(masks)
    with pytest.raises(ValueError, match="query 0"):
        idx.search_batch(Q, 31, filter=qf)                    # k > |F_0|
    ids, sc = idx.search_batch(Q, 20, filter=qf)              # query 0: |F_0| < 2k, query 2: empty
    assert np.all(ids[2] == -1) and np.all(np.isnan(sc[2]))
    for j in (0, 1):
        want = idx.search_batch(Q[j:j + 1], 20, filter=idx.make_filter(masks[j]))
        assert _same((ids[j:j + 1], sc[j:j + 1]), want), j
    k0 = idx.search_batch(Q, 0, filter=qf)
    assert k0[0].shape == (3, 0) and k0[1].shape == (3, 0)
    # an unprepared [B, N] bool mask, doc-id lists and row lists name the same filters
    a = idx.search_batch(Q, 5, filter=masks)
    assert _same(a, idx.search_batch(Q, 5, filter=qf))
    lists = [np.nonzero(m)[0] for m in masks]
    assert _same(idx.search_batch(Q, 5, filter=idx.make_query_filters(rows=lists)), a)
    assert _same(idx.search_batch(Q, 5, filter=idx.make_query_filters(doc_ids=[[f"d{i}" for i in r] for r in lists])), a)
    # search: a set of one list
    one = idx.make_query_filters(masks[:1])
    assert [x[:2] for x in idx.search(Q[0], 5, filter=one)] == [x[:2] for x in idx.search(Q[0], 5, filter=masks[0])]
    assert idx.search(Q[0], 5, filter=idx.make_query_filters(masks[2:3])) == []
    with pytest.raises(ValueError):
        idx.search_batch(Q[:2], 5, filter=qf)                 # n_queries != B
    with pytest.raises(ValueError):
        idx.make_query_filters(np.ones((2, n - 1), bool))     # wrong length
    with pytest.raises(ValueError):
        idx.make_query_filters(np.ones((2, n), np.int32))     # not boolean
    with pytest.raises(KeyError):
        idx.make_query_filters(doc_ids=[["d1"], ["nope"]])
    with pytest.raises(ValueError):
        idx.make_query_filters(rows=[[0, 1], [n]])
    # stale after a rebuild
    from dewi.types import Payload
    idx.add("extra", raw[0], Payload())
    idx.build()
    with pytest.raises(ValueError):
        idx.search_batch(Q, 5, filter=qf)


def test_query_filters_stale_after_load(tmp_path):
    from dewi.backends import ExactIndex
    idx, raw, _ = _index(n=400)
    masks = np.ones((2, 400), bool)
    qf = idx.make_query_filters(masks)
    idx.save(tmp_path / "i")
    other = ExactIndex.load(tmp_path / "i")
    with pytest.raises(ValueError):
        other.search_batch(raw[:2], 5, filter=qf)
    assert other.search_batch(raw[:2], 5, filter=other.make_query_filters(masks))[0].shape == (2, 5)


def test_query_filters_bf16_unsupported():
    c, _, _, _ = _corpus(1000, 256, "cosine", seed=1)
    cb = c.to_bf16()
    qf = cb.make_query_filters(np.ones((2, 1000), bool))
    with pytest.raises(NotImplementedError):
        cb.search(orc.synth_queries(2, 256, seed=2), 5, 0.3, 0.0, filter=qf)


def test_dewi_index_forwards_query_filters():
    from dewi.index import DewiIndex
    from dewi.types import payloads_from_columns
    n, d = 800, 64
    raw = orc.synth_corpus(n, d, seed=8)
    cols = orc.synth_payload_columns(n, seed=8)
    index = DewiIndex(dim=d, use_ann=False, rerank_eta=0.3)
    index.add_batch([f"x{i}" for i in range(n)], raw, payloads_from_columns(cols))
    keep7 = [f"x{i}" for i in range(0, n, 7)]
    keep3 = [f"x{i}" for i in range(0, n, 3)]
    qf = index.make_query_filters(doc_ids=[keep7, keep3, []])
    rb = index.search_batch(raw[[14, 21, 5]], 5, filter=qf)
    assert rb[0][0][0] == "x14" and all(doc in keep7 for doc, _, _ in rb[0])
    assert rb[1][0][0] == "x21" and all(doc in keep3 for doc, _, _ in rb[1])
    assert rb[2] == []
    assert [x[:2] for x in rb[0]] == [x[:2] for x in index.search(raw[14], 5, filter=keep7)]
    assert [x[:2] for x in rb[1]] == [x[:2] for x in index.search(raw[21], 5, filter=keep3)]


# ---------------------------------------------------------------------------------------------------------------- 6. full size
def test_query_filters_full_size():
    n, dim, k, b = 1 << 20, 768, 10, 32
    c, E, dewi32, ent32 = _corpus(n, dim, "cosine", seed=42)
    rs = np.random.RandomState(5)
    masks = rs.rand(b, n) < rs.uniform(0.08, 0.12, size=(b, 1))
    Q = orc.synth_queries(b, dim, seed=7)
    ids, sc = c.search(Q, k, 0.3, 0.0, filter=c.make_query_filters(masks))
    dec = 0
    for j in range(b):
        rows = np.nonzero(masks[j])[0]
        pos = np.searchsorted(rows, ids[j])
        assert np.array_equal(rows[np.minimum(pos, rows.size - 1)], ids[j]), f"query {j}: an id outside its list"
        decisive, msg = compare_query(E[rows], Q[j], dewi32[rows], ent32[rows], k, 0.3, 0.0, "cosine", pos, sc[j])
        assert msg is None, f"query {j}: {msg}"
        dec += int(decisive)
    assert dec >= 0.75 * b, f"only {dec}/{b} decisive queries"
    for j in (0, 9, 18, 31):
        want = c.search(Q[j:j + 1], k, 0.3, 0.0, filter=c.make_filter(masks[j]))
        assert _same((ids[j:j + 1], sc[j:j + 1]), want), j


# ---------------------------------------------------------------------------------------------------------------- 7. tuning
def test_query_filters_workspace_follows_tuning():
    """As ``test_filtered_workspace_follows_tuning`` for per-query lists: two lists of 8192 rows each share one pass, whose
    workspace is sized from the calling thread's launch plan — after ``tuning()`` it is asked for again and grown."""
    eng = _eng()
    n, dim, k, b = 16384, 256, 10, 2
    masks = np.zeros((b, n), bool)
    masks[0, ::2] = True                                               # 8192 rows
    masks[1, :8192] = True                                             # 8192 rows, half of them the other list's
    Q = orc.synth_queries(b, dim, seed=99)
    c, _, _, _ = _corpus(n, dim, "cosine", seed=98)
    qf = c.make_query_filters(masks)
    assert qf.n_allowed.tolist() == [8192, 8192] and qf.n_union == 12288
    try:
        eng.tuning(scan_blocks=8)
        need_8 = [int(c._lib.dewi_knn_filtered_workspace_bytes(8192, dim, b, 2 * k)),
                  int(c._lib.dewi_knn_query_filtered_workspace_bytes(qf.n_union, dim, b, 2 * k))]
        c.search(Q, k, 0.3, 0.0, filter=qf)
        eng.tuning()
        need_default = [int(c._lib.dewi_knn_filtered_workspace_bytes(8192, dim, b, 2 * k)),
                        int(c._lib.dewi_knn_query_filtered_workspace_bytes(qf.n_union, dim, b, 2 * k))]
        print(f"query-filtered workspace: {need_8} B under scan_blocks=8, {need_default} B under the defaults")
        assert need_8[0] != need_default[0] and need_8[1] != need_default[1] and min(need_8 + need_default) > 0
        got = c.search(Q, k, 0.3, 0.0, filter=qf)
    finally:
        eng.tuning()
    fresh, _, _, _ = _corpus(n, dim, "cosine", seed=98)
    want = fresh.search(Q, k, 0.3, 0.0, filter=fresh.make_query_filters(masks))
    assert got[0].shape == (b, k) and _same(got, want)

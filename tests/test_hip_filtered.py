"""GPU tests of the filtered search (ABI 6): ``search(..., filter=...)`` restricted to an allow-list A of rows.

Contract: a filtered search is the reference's ExactIndex.search (src/dewi/backends.py:414-481) applied to the rows of A only.
The oracle is therefore ``dewi_oracle`` on E[A], with its ids mapped back through the sorted list of A (a monotone map: the
tie rule carries over).  On top of that, a row of A is scored with exactly the arithmetic of the unfiltered one-query search
(the LIST forms of the same row kernels), so a filter that contains a query's unfiltered candidates must give that query's
unfiltered result bit for bit.
"""
import numpy as np
import pytest

import dewi_oracle as orc
from parity import check_batch, compare_query

pytestmark = pytest.mark.gpu

FAST_DIMS = [256, 768, 1536]
ANY_DIMS = [384, 1000, 1280, 3072, 4096]
SHORT_DIMS = [64, 100]
ODD_DIMS = [5, 50, 129, 301, 1001, 3001]
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


def _masks(n, dim, seed):
    rs = np.random.RandomState(seed)
    g = max(_period(dim), 4)
    out = {
        "all": np.ones(n, bool),
        "rand30": rs.rand(n) < 0.30,
        "rand1": rs.rand(n) < 0.01,
        "block": np.zeros(n, bool),
        "residue": (np.arange(n) % g) == 1,
        "first_last": np.zeros(n, bool),
        "single": np.zeros(n, bool),
        "empty": np.zeros(n, bool),
    }
    out["block"][n // 3: n // 3 + n // 5] = True
    out["first_last"][[0, n - 1]] = True
    out["single"][n // 2 + 1] = True
    return out


def _corpus(n, dim, space, seed):
    raw = orc.synth_corpus(n, dim, seed=seed)
    cols = orc.synth_payload_columns(n, seed=seed)
    c = _eng().DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    return c, c.emb.cpu().numpy(), dewi32, ent32


def _check_on_subset(E, rows, Q, dewi32, ent32, k, eta, pref, space, ids, sc):
    """Oracle on E[rows]; returns the number of decisive queries."""
    if rows.size == 0 or k <= 0:
        assert ids.shape == (Q.shape[0], 0) and sc.shape == (Q.shape[0], 0)
        return 0
    pos = np.searchsorted(rows, ids)
    assert np.all(pos < rows.size) and np.array_equal(rows[np.minimum(pos, rows.size - 1)], ids), "an id outside the filter"
    n_dec = 0
    for j in range(Q.shape[0]):
        decisive, msg = compare_query(E[rows], Q[j], dewi32[rows], ent32[rows], k, eta, pref, space, pos[j], sc[j])
        assert msg is None, f"query {j}: {msg}"
        n_dec += int(decisive)
    return n_dec


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 1. oracle
@pytest.mark.parametrize("dim", ALL_DIMS)
def test_filtered_oracle_parity(dim):
    n = 2003 if dim <= 1600 else 1201
    total = dec = 0
    for space in ("cosine", "l2"):
        c, E, dewi32, ent32 = _corpus(n, dim, space, seed=dim + (7 if space == "l2" else 0))
        Q = orc.synth_queries(9, dim, seed=dim + 3)
        for name, mask in _masks(n, dim, seed=dim).items():
            rows = np.nonzero(mask)[0]
            f = c.make_filter(mask)
            assert f.n_allowed == rows.size, name
            k = min(10, rows.size)
            ids, sc = c.search(Q, k, 0.3, 0.0, filter=f)               # 9 queries: 8 + 1 (fast) or 4 + 4 + 1 passes
            dec += _check_on_subset(E, rows, Q, dewi32, ent32, k, 0.3, 0.0, space, ids, sc)
            total += Q.shape[0] if rows.size else 0
            for b in (1, 3, 4):                                          # other pass mixes: the same answers
                got = c.search(Q[:b], k, 0.3, 0.0, filter=f)
                assert _same(got, (ids[:b], sc[:b])), (space, name, b)
        # a larger cut (per-wave lists, dense keys) on the 30 % filter
        rows = np.nonzero(_masks(n, dim, seed=dim)["rand30"])[0]
        f = c.make_filter(rows_mask(n, rows))
        for k in (100, 150):
            ids, sc = c.search(Q[:4], k, 0.5, 0.2, filter=f)
            _check_on_subset(E, rows, Q[:4], dewi32, ent32, k, 0.5, 0.2, space, ids, sc)
    assert dec >= 0.5 * total, f"only {dec}/{total} decisive queries"


def rows_mask(n, rows):
    m = np.zeros(n, bool)
    m[rows] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- 2. bits
def _topc_superset(E, Q, k, space, extra):
    """CPU: every row within the f64 top (c + extra) of some query — a superset of the unfiltered candidates."""
    rows = set()
    for q in Q:
        qp = orc.prepare_query(q, space).astype(np.float64)
        E64 = E.astype(np.float64)
        s = E64 @ qp if space != "l2" else -np.sum((E64 - qp[None, :]) ** 2, axis=1)
        s = np.where(np.isnan(s), np.inf, s)
        rows.update(np.argsort(-s, kind="stable")[: 2 * k + extra].tolist())
    return rows


@pytest.mark.parametrize("dim", ALL_DIMS)
def test_filtered_equals_unfiltered_bits(dim):
    n = 2003 if dim <= 1600 else 1201
    k = 10
    for space in ("cosine", "l2"):
        c, E, _, _ = _corpus(n, dim, space, seed=dim + 11)
        Q = orc.synth_queries(5, dim, seed=dim + 13)
        rs = np.random.RandomState(dim)
        for j in range(Q.shape[0]):
            want = c.search(Q[j:j + 1], k, 0.3, 0.1)
            rows = _topc_superset(E, Q[j:j + 1], k, space, 40) | set(rs.choice(n, n // 10, replace=False).tolist())
            got = c.search(Q[j:j + 1], k, 0.3, 0.1, filter=c.make_filter(rows_mask(n, sorted(rows))))
            assert _same(got, want), (space, j)
        f_all = c.make_filter(np.ones(n, bool))
        for j in range(Q.shape[0]):
            assert _same(c.search(Q[j:j + 1], k, 0.3, 0.1, filter=f_all), c.search(Q[j:j + 1], k, 0.3, 0.1)), (space, j)


# ---------------------------------------------------------------------------------------------------------------- 3. batch
@pytest.mark.parametrize("dim", [100, 301, 768, 1000, 4100, 4101])
def test_filtered_batch_equals_singles(dim):
    n = 3001
    for space in ("cosine", "l2"):
        c, _, _, _ = _corpus(n, dim, space, seed=dim + 21)
        Q = orc.synth_queries(33, dim, seed=dim + 23)
        f = c.make_filter(np.random.RandomState(dim).rand(n) < 0.4)
        singles = [c.search(Q[j:j + 1], 10, 0.3, 0.0, filter=f) for j in range(33)]
        for b in (2, 4, 5, 8, 33):
            ids, sc = c.search(Q[:b], 10, 0.3, 0.0, filter=f)
            for j in range(b):
                assert _same((ids[j:j + 1], sc[j:j + 1]), singles[j]), (space, b, j)


# ---------------------------------------------------------------------------------------------------------------- 4. leaks
@pytest.mark.parametrize("dim", [5, 50, 129, 301, 1001])
def test_filtered_neighbours_do_not_leak(dim):
    n = 1601
    rs = np.random.RandomState(dim)
    raw = orc.synth_corpus(n, dim, seed=dim + 31)
    allowed = np.zeros(n, bool)
    allowed[rs.choice(n, n // 4, replace=False)] = True
    poison = np.nonzero(~allowed & (np.roll(allowed, 1) | np.roll(allowed, -1)))[0]   # right next to an allowed row
    raw[poison[::2]] = np.nan
    raw[poison[1::2]] = 1e30
    cols = orc.synth_payload_columns(n, seed=dim)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    rows = np.nonzero(allowed)[0]
    Q = orc.synth_queries(6, dim, seed=dim + 33)
    for space in ("cosine", "l2"):
        c = _eng().DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space)
        E = c.emb.cpu().numpy()
        ids, sc = c.search(Q, 10, 0.3, 0.0, filter=c.make_filter(allowed))
        check_batch(E[rows], Q, dewi32[rows], ent32[rows], 10, 0.3, 0.0, space, np.searchsorted(rows, ids), sc,
                    min_decisive_frac=0.5)
        # a shard view whose first row does not start on a 16-byte unit (row 1 of the buffer): the same answers
        sub = _eng().DeviceCorpus(c.emb[1:], c.dewi32[1:], c.ent32[1:], space)
        rows1 = rows[rows >= 1] - 1
        ids1, sc1 = sub.search(Q, 10, 0.3, 0.0, filter=sub.make_filter(allowed[1:]))
        check_batch(E[1:][rows1], Q, dewi32[1:][rows1], ent32[1:][rows1], 10, 0.3, 0.0, space, np.searchsorted(rows1, ids1),
                    sc1, min_decisive_frac=0.5)


@pytest.mark.parametrize("dim", [100, 301, 768])
def test_filtered_zero_norm_rows_inside(dim):
    """Zero rows of a cosine corpus are NaN after normalisation: they stay in the cut and in the top k and come last, as in
    the reference (``argsort(-adjusted)`` sorts NaN to the end), unfiltered as filtered."""
    n = 2003
    raw = orc.synth_corpus(n, dim, seed=dim + 41)
    raw[[3, 500, 1999]] = 0.0
    cols = orc.synth_payload_columns(n, seed=dim)
    c = _eng().DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    E = c.emb.cpu().numpy()
    Q = orc.synth_queries(3, dim, seed=dim + 43)
    for j in range(3):
        want = c.search(Q[j:j + 1], 10, 0.3, 0.0)
        rows = _topc_superset(E, Q[j:j + 1], 10, "cosine", 30) | {3, 500, 1999, 7, 8, 9}
        got = c.search(Q[j:j + 1], 10, 0.3, 0.0, filter=c.make_filter(rows_mask(n, sorted(rows))))
        assert _same(got, want), j
        assert set(got[0][0, 7:].tolist()) == {3, 500, 1999} and np.isnan(got[1][0, 7:]).all()
        assert not np.isnan(got[1][0, :7]).any()


# ---------------------------------------------------------------------------------------------------------------- 5. rules
def _index(n=1500, dim=96, space="cosine", **kw):
    from dewi.backends import ExactIndex
    from dewi.types import payloads_from_columns
    raw = orc.synth_corpus(n, dim, seed=5)
    cols = orc.synth_payload_columns(n, seed=5)
    idx = ExactIndex(dim, space, **kw)
    idx.add_batch([f"d{i}" for i in range(n)], raw, payloads_from_columns(cols))
    idx.build()
    return idx, raw, cols


def test_filtered_rules():
    idx, raw, cols = _index()
    n = raw.shape[0]
    q = orc.synth_queries(1, raw.shape[1], seed=9)[0]
    mask = np.zeros(n, bool)
    mask[::50] = True                                        # 30 rows
    f = idx.make_filter(mask)
    assert idx.search(q, 0, filter=f) == []
    assert idx.search(q, -3, filter=f) == []
    assert idx.search(q, 5, filter=idx.make_filter(np.zeros(n, bool))) == []
    ids, sc = idx.search_batch(np.stack([q, q]), 5, filter=np.zeros(n, bool))
    assert ids.shape == (2, 0) and sc.shape == (2, 0)
    with pytest.raises(ValueError):
        idx.search(q, 31, filter=f)                          # k > |A|
    assert len(idx.search(q, 30, filter=f)) == 30
    # candidates=k with each similarity transform: ids inside the filter, equal to the unfiltered rule on E[A]
    for sim in ("ip", "one_minus_dist", "inv_one_plus_dist"):
        r = idx.search(q, 5, candidates=5, similarity=sim, filter=f)
        assert len(r) == 5 and all(int(d[1:]) % 50 == 0 for d, _, _ in r), sim
    with pytest.raises(ValueError):
        idx.make_filter(np.ones(n - 1, bool))                # wrong length
    with pytest.raises(ValueError):
        idx.search(q, 5, filter=np.ones(n + 1, bool))
    with pytest.raises(KeyError):
        idx.make_filter(doc_ids=["d1", "nope"])
    # doc ids, rows and a mask name the same filter
    a = idx.search(q, 5, filter=idx.make_filter(doc_ids=[f"d{i}" for i in range(0, n, 50)]))
    b = idx.search(q, 5, filter=idx.make_filter(rows=np.arange(0, n, 50)))
    assert [x[:2] for x in a] == [x[:2] for x in b] == [x[:2] for x in idx.search(q, 5, filter=f)]
    # stale: the index was rebuilt since the filter was prepared
    from dewi.types import Payload
    idx.add("extra", raw[0], Payload())
    idx.build()
    with pytest.raises(ValueError):
        idx.search(q, 5, filter=f)


def test_filtered_stale_after_load(tmp_path):
    from dewi.backends import ExactIndex
    idx, raw, _ = _index(n=400)
    f = idx.make_filter(np.ones(400, bool))
    idx.save(tmp_path / "i")
    other = ExactIndex.load(tmp_path / "i")
    with pytest.raises(ValueError):
        other.search(raw[1], 5, filter=f)
    assert len(other.search(raw[1], 5, filter=other.make_filter(np.ones(400, bool)))) == 5


def test_filtered_batch_shadow_takes_rows():
    idx, raw, cols = _index(n=70000, dim=256, batch_shadow=True)
    plain, _, _ = _index(n=70000, dim=256)
    Q = orc.synth_queries(8, 256, seed=3)
    mask = np.random.RandomState(1).rand(70000) < 0.2
    a = idx.search_batch(Q, 10, filter=mask)
    b = plain.search_batch(Q, 10, filter=mask)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_filtered_bf16_unsupported():
    c, _, _, _ = _corpus(1000, 256, "cosine", seed=1)
    cb = c.to_bf16()
    f = cb.make_filter(np.ones(1000, bool))
    with pytest.raises(NotImplementedError):
        cb.search(orc.synth_queries(1, 256, seed=2), 5, 0.3, 0.0, filter=f)


def test_dewi_index_forwards_filter():
    from dewi.index import DewiIndex
    from dewi.types import payloads_from_columns
    n, d = 800, 64
    raw = orc.synth_corpus(n, d, seed=8)
    cols = orc.synth_payload_columns(n, seed=8)
    index = DewiIndex(dim=d, use_ann=False, rerank_eta=0.3)
    index.add_batch([f"x{i}" for i in range(n)], raw, payloads_from_columns(cols))
    keep = [f"x{i}" for i in range(0, n, 7)]
    f = index.make_filter(doc_ids=keep)
    r = index.search(raw[14], 5, filter=f)
    assert r[0][0] == "x14" and all(doc in keep for doc, _, _ in r)
    rb = index.search_batch(raw[[14, 21]], 5, filter=keep)
    assert [x[:2] for x in rb[0]] == [x[:2] for x in r]


# ---------------------------------------------------------------------------------------------------------------- 6. full size
def test_filtered_full_size():
    n, dim, k = 1 << 20, 768, 10
    c, E, dewi32, ent32 = _corpus(n, dim, "cosine", seed=42)
    mask = np.random.RandomState(5).rand(n) < 0.10
    rows = np.nonzero(mask)[0]
    Q = orc.synth_queries(32, dim, seed=7)
    ids, sc = c.search(Q, k, 0.3, 0.0, filter=c.make_filter(mask))
    check_batch(E[rows], Q, dewi32[rows], ent32[rows], k, 0.3, 0.0, "cosine", np.searchsorted(rows, ids), sc,
                min_decisive_frac=0.75)


# ---------------------------------------------------------------------------------------------------------------- 7. tuning
def test_filtered_workspace_follows_tuning():
    """The workspace of a filtered search is sized from the calling thread's launch plan: a corpus that served the search
    under ``tuning(scan_blocks=8)`` (8 lists per query) serves it again under the defaults (8192 listed rows at dim 256: 64
    workgroups, 64 lists) — asked for again and grown, not reused too small — and answers as a fresh corpus does."""
    eng = _eng()
    n, dim, k, b = 16384, 256, 10, 3
    mask = rows_mask(n, np.arange(0, n, 2))                            # 8192 rows
    Q = orc.synth_queries(b, dim, seed=97)
    c, _, _, _ = _corpus(n, dim, "cosine", seed=95)
    f = c.make_filter(mask)
    assert f.n_allowed == 8192
    try:
        eng.tuning(scan_blocks=8)
        need_8 = int(c._lib.dewi_knn_filtered_workspace_bytes(8192, dim, b, 2 * k))
        c.search(Q, k, 0.3, 0.0, filter=f)
        eng.tuning()
        need_default = int(c._lib.dewi_knn_filtered_workspace_bytes(8192, dim, b, 2 * k))
        print(f"filtered workspace: {need_8} B under scan_blocks=8, {need_default} B under the defaults")
        assert need_8 != need_default and need_8 > 0 and need_default > 0
        got = c.search(Q, k, 0.3, 0.0, filter=f)
    finally:
        eng.tuning()
    fresh, _, _, _ = _corpus(n, dim, "cosine", seed=95)
    want = fresh.search(Q, k, 0.3, 0.0, filter=fresh.make_filter(mask))
    assert got[0].shape == (b, k) and _same(got, want)

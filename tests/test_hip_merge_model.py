"""GPU: the merge / re-rank stage (``merge_rerank_kernel``, ``merge_rerank_large_kernel`` and the three branches of
``rerank_and_emit``) against tests/rerank_model.py, bit for bit, on records built on the host.

The stage is a pure function of 16-byte records and every operation of the blend has one defined fp32 rounding, so there are
no tolerances: ids equal, scores ``array_equal(equal_nan=True)``, and the caller's prefill (ids -7, scores 123.0 here) intact
from ``kk = min(k, n_candidates, n_valid)`` on.  Each list is sorted by (sim desc, id asc) with its padding at the tail, as the
ABI requires; ids are unique inside a query.  The shapes sit on the route boundaries of the launchers: 256 records (ranking
pass / bitonic sort), 512 records (256 / 1024 threads), 2048 records (LDS / global rank-merge), and ``n_sel`` 64 and 256
inside ``rerank_and_emit`` (one lane per candidate / lane groups / bitonic)."""
import numpy as np
import pytest

import rerank_model as rm

pytestmark = pytest.mark.gpu

B = 3
# (n_lists, list_len, n_candidates, k)
SHAPES = [
    (2, 20, 20, 10), (8, 32, 256, 128), (1, 5, 5, 5),                     # ranking pass, 256 threads
    (1, 257, 200, 100), (8, 64, 200, 10),                                 # bitonic with 256 threads (257 / 512 records)
    (3, 171, 65, 65), (8, 100, 100, 50), (8, 256, 256, 256), (8, 256, 257, 200), (8, 256, 2048, 1024),   # 1024 threads
    (1, 2049, 2049, 1025), (8, 400, 400, 200), (8, 3000, 3000, 1500), (3, 1000, 700, 700),               # global rank-merge
]
# (eta, pref): adjusted ties at eta = 1 (dewi from four values), the similarity alone at eta = 0 (and 0 * inf), with / without ent
BLENDS = [(1.0, 0.0), (0.0, 0.0), (0.3, 0.25), (0.3, 0.0), (0.0, -0.5)]
CONTENTS = ["ties", "special", "mostly_nan", "ragged", "short"]


def _ids(rs, m):
    """m distinct ids for one query: 0, 1 and 2^31 - 1 among them (where they fit)."""
    pool = rs.choice(np.arange(2, 16 * m + 64), size=m, replace=False).astype(np.int64)
    special = [0, 1, 2 ** 31 - 1][: min(3, m)]
    pool[rs.choice(m, len(special), replace=False)] = special
    return pool.astype(np.int32)


def make_lists(content, n_lists, list_len, k, seed):
    """Structured records [n_lists][B][list_len] for one content kind."""
    rs = np.random.RandomState(seed)
    m = n_lists * list_len
    lists = np.zeros((n_lists, B, list_len), rm.RECORD)
    for q in range(B):
        sim = rs.choice(np.array([0.75, 0.5, 0.25, 0.0, -0.5], np.float32), m)       # ties across lists; the cut falls inside one
        dewi = rs.choice(np.array([0.125, 0.25, 0.5, 0.875], np.float32), m)
        ent = rs.rand(m).astype(np.float32)
        valid = np.full(n_lists, list_len)
        if content == "special":
            sim = np.where(rs.rand(m) < 0.5, sim, rs.randn(m)).astype(np.float32)
            sim[rs.rand(m) < 0.10] = -0.0
            sim[rs.rand(m) < 0.05] = -np.inf
            sim[rs.rand(m) < 0.04] = np.nan
            dewi[rs.rand(m) < 0.04] = np.nan
            dewi[rs.rand(m) < 0.04] = np.inf                  # eta = 0: 0 * inf
            dewi[rs.rand(m) < 0.04] = -np.inf
            ent[rs.rand(m) < 0.04] = np.nan                   # counts only with pref != 0
        elif content == "mostly_nan":                         # more NaN adjusted scores than kk
            sim = rs.randn(m).astype(np.float32)
            sim[rs.rand(m) < 0.3] = np.nan
            dewi[rs.rand(m) < 0.9] = np.nan
        elif content == "ragged":                             # ragged valid counts, one list all padding (where there are two)
            valid = rs.randint(0, list_len + 1, n_lists)
            valid[rs.randint(n_lists)] = list_len if n_lists == 1 else 0
            if q == 1:
                sim = rs.randn(m).astype(np.float32)
                dewi[rs.rand(m) < 0.02] = np.nan
        elif content == "short":                              # n_valid < k (and < n_candidates)
            total = max(1, k // 2) if q else max(1, k - 1)
            valid = np.bincount(rs.randint(0, n_lists, total), minlength=n_lists)
            valid = np.minimum(valid, list_len)
            if q == 2:
                dewi[rs.rand(m) < 0.3] = np.nan
        ids = _ids(rs, m)
        for l in range(n_lists):
            recs = np.zeros(list_len, rm.RECORD)
            sl = slice(l * list_len, (l + 1) * list_len)
            recs["sim"], recs["dewi"], recs["ent"], recs["id"] = sim[sl], dewi[sl], ent[sl], ids[sl]
            recs["id"][valid[l]:] = -1
            order = rm.record_order(recs)                     # (ord(sim) desc, id asc): NaN first, -0 == +0
            lists[l, q, : order.shape[0]] = recs[order]
            lists[l, q, order.shape[0]:] = (-np.inf, 0.0, 0.0, -1)
    return lists


def run_device(lists, n_candidates, k, eta, pref):
    import torch
    from dewi import _engine as eng
    recs = torch.from_numpy(np.ascontiguousarray(lists).view(np.int32).reshape(lists.shape + (4,))).cuda()
    out_ids = torch.full((lists.shape[1], k), -7, dtype=torch.int64, device="cuda")
    out_sc = torch.full((lists.shape[1], k), 123.0, dtype=torch.float32, device="cuda")
    eng.merge_rerank_device(recs, n_candidates, k, eta, pref, out_ids=out_ids, out_scores=out_sc)
    return out_ids.cpu().numpy(), out_sc.cpu().numpy()


def check(lists, n_candidates, k, eta, pref):
    want_ids, want_sc = rm.merge_rerank(lists, n_candidates, k, eta, pref, np.full((B, k), -7, np.int64),
                                        np.full((B, k), 123.0, np.float32))
    ids, sc = run_device(lists, n_candidates, k, eta, pref)
    for q in range(B):
        first = int(np.argmax(ids[q] != want_ids[q])) if (ids[q] != want_ids[q]).any() else -1
        assert first < 0, (f"query {q} eta {eta} pref {pref}: ids differ from position {first}: got {ids[q, first:first + 6].tolist()} "
                           f"{sc[q, first:first + 6].tolist()} want {want_ids[q, first:first + 6].tolist()} "
                           f"{want_sc[q, first:first + 6].tolist()}")
        assert np.array_equal(sc[q], want_sc[q], equal_nan=True), f"query {q} eta {eta} pref {pref}: scores differ"
    return want_ids, want_sc


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_rerank_equals_the_model(shape, content):
    n_lists, list_len, n_candidates, k = shape
    lists = make_lists(content, n_lists, list_len, k, seed=1000 * SHAPES.index(shape) + CONTENTS.index(content))
    n_valid = (lists["id"] >= 0).sum(axis=(0, 2))
    if content == "short":
        assert (n_valid < k).all()
    for eta, pref in BLENDS:
        want_ids, want_sc = check(lists, n_candidates, k, eta, pref)
        for q in range(B):
            kk = min(k, n_candidates, int(n_valid[q]))
            assert (want_ids[q, kk:] == -7).all() and (want_sc[q, kk:] == 123.0).all()      # the prefill, from kk on
            assert (want_ids[q, :kk] >= 0).all()
            nan = np.isnan(want_sc[q, :kk])
            assert not nan[: kk - int(nan.sum())].any()                                     # the model itself: NaN scores last
    if content == "mostly_nan" and k < n_candidates:
        assert np.isnan(want_sc[:, :min(k, n_candidates)]).all()                            # more NaN scores than kk: only NaN comes back


@pytest.mark.parametrize("shape", [(2, 20, 20, 10), (8, 64, 200, 10), (8, 256, 2048, 1024), (8, 400, 400, 200)],
                         ids=lambda s: "x".join(map(str, s)))
def test_a_refused_query_is_marked_and_its_neighbours_are_answered(shape):
    """A -2 record (a shard could not answer the query) in ONE query of the batch: that row is -1 / NaN over all k positions,
    the other queries are answered as the model answers them."""
    n_lists, list_len, n_candidates, k = shape
    lists = make_lists("special", n_lists, list_len, k, seed=77 + n_lists * list_len)
    lists[n_lists - 1, 1, :] = (np.nan, 0.0, 0.0, -2)         # as the shard select writes a refused query's records
    want_ids, want_sc = check(lists, n_candidates, k, 0.3, 0.25)
    assert (want_ids[1] == -1).all() and np.isnan(want_sc[1]).all()
    assert (want_ids[[0, 2], 0] >= 0).all()
    lists[n_lists - 1, 1, :] = (-np.inf, 0.0, 0.0, -1)
    lists[0, 1, list_len - 1] = (np.nan, 0.0, 0.0, -2)        # a single marker, at a list's tail
    want_ids, _ = check(lists, n_candidates, k, 0.3, 0.0)
    assert (want_ids[1] == -1).all()

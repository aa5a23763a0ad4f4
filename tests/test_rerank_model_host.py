"""CPU: tests/rerank_model.py (the model the GPU merge / re-rank tests compare with) pinned to the oracle.

One list holds every row of a corpus as a (sim, dewi32, ent32, row) record, sorted by the record key.  ``merge_rerank`` with
``n_candidates = 2k`` is then the oracle's whole search after the similarities: it must return ``orc.search``'s ids id for id
and its scores bit for bit on corpora without ties; with NaN rows or NaN payload values the numbers in front must be equal in
the same way, the NaN tail equal as a set (its internal order is an artefact of NumPy's introselect in the reference)."""
import numpy as np
import pytest

import dewi_oracle as orc
import rerank_model as rm


def _records(E, q, dewi32, ent32, space):
    s = orc.similarities(E, orc.prepare_query(q, space), space).astype(np.float32)
    recs = np.zeros(E.shape[0], rm.RECORD)
    recs["sim"], recs["dewi"], recs["ent"], recs["id"] = s, dewi32, ent32, np.arange(E.shape[0])
    return recs[rm.record_order(recs)][None, None, :]


def _corpus(n, dim, seed, space):
    rs = np.random.RandomState(seed)
    raw = rs.randn(n, dim).astype(np.float32)
    cols = orc.synth_payload_columns(n, seed=seed)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    return raw, dewi32, ent32, rs.randn(4, dim).astype(np.float32)


def test_ord32_orders_like_the_device_key():
    x = np.array([np.nan, np.inf, 3.0, 1e-45, 0.0, -0.0, -1e-45, -2.0, -np.inf], np.float32)
    key = rm.ord32(x)
    assert key[0] == 0xFFFFFFFF and key[4] == key[5]
    assert np.all(key[:4].astype(np.int64) > key[1:5].astype(np.int64))
    assert np.all(key[5:-1].astype(np.int64) > key[6:].astype(np.int64))


@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("n,dim,k,eta,pref", [(300, 32, 5, 0.3, 0.0), (500, 48, 40, 0.5, 0.2), (64, 16, 64, 0.0, -0.3),
                                              (200, 24, 150, 1.0, 0.0), (7, 8, 3, 0.7, 0.1)])
def test_model_equals_oracle_without_ties(space, n, dim, k, eta, pref):
    raw, dewi32, ent32, Q = _corpus(n, dim, 11 + n, space)
    E = orc.build_matrix(raw, space)
    for q in Q:
        want_ids, want_sc = orc.search(E, q, dewi32, ent32, k, eta, pref, space)
        ids, sc = rm.merge_rerank(_records(E, q, dewi32, ent32, space), 2 * k, k, eta, pref)
        assert np.array_equal(ids[0], want_ids)
        assert np.array_equal(sc[0].view(np.uint32), want_sc.view(np.uint32))


@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("n_nan_rows,n_nan_dewi,n_nan_ent,k,eta,pref", [
    (1, 0, 0, 5, 0.3, 0.0), (5, 0, 0, 5, 0.3, 0.0), (2, 2, 0, 8, 0.4, 0.0), (0, 3, 0, 6, 0.5, 0.0), (0, 0, 3, 6, 0.5, 0.25),
    (1, 1, 1, 3, 0.2, -0.1), (3, 0, 0, 40, 0.3, 0.0)])
def test_model_equals_oracle_with_nan_scores(space, n_nan_rows, n_nan_dewi, n_nan_ent, k, eta, pref):
    """1 .. k NaN adjusted scores among the candidates: zero rows (cosine) / NaN rows (l2), and NaN payload values planted on
    rows inside the candidate cut of every query (ent only counts with pref != 0)."""
    n, dim = 300, 32
    raw, dewi32, ent32, Q = _corpus(n, dim, 23 + k, space)
    rows = np.random.RandomState(k).choice(n, n_nan_rows, replace=False)
    raw[rows] = 0.0 if space == "cosine" else np.nan
    E = orc.build_matrix(raw, space)
    for q in Q:
        d, e = dewi32.copy(), ent32.copy()
        s = orc.similarities(E, orc.prepare_query(q, space), space)
        inside = [int(r) for r in np.argsort(-np.where(np.isnan(s), -np.inf, s))[: 2 * k - n_nan_rows - 1]]
        d[inside[1: 1 + n_nan_dewi]] = np.nan
        e[inside[4: 4 + n_nan_ent]] = np.nan
        planted = set(rows.tolist()) | set(inside[1: 1 + n_nan_dewi]) | set(inside[4: 4 + n_nan_ent])
        assert 1 <= len(planted) <= k
        want_ids, want_sc = orc.search(E, q, d, e, k, eta, pref, space)
        ids, sc = rm.merge_rerank(_records(E, q, d, e, space), 2 * k, k, eta, pref)
        z = len(planted)
        assert np.isnan(want_sc[k - z:]).all() and not np.isnan(want_sc[: k - z]).any()      # the reference: NaN last
        assert np.array_equal(ids[0, : k - z], want_ids[: k - z])
        assert set(ids[0, k - z:].tolist()) == set(want_ids[k - z:].tolist()) == planted
        assert np.array_equal(sc[0], want_sc, equal_nan=True)
        assert np.array_equal(sc[0, : k - z].view(np.uint32), want_sc[: k - z].view(np.uint32))


def test_model_contract_details():
    recs = np.zeros((2, 2, 4), rm.RECORD)
    recs["id"] = -1
    recs["sim"] = -np.inf
    # query 0: two lists, a cross-list tie on sim (lower id first), -0 == +0, a NaN sim on top, padding at the tails
    recs[0, 0, :3] = [(np.nan, 0.5, 0.0, 9), (1.0, 0.0, 0.0, 7), (-0.0, 1.0, 0.0, 4)]
    recs[1, 0, :2] = [(1.0, 0.0, 0.0, 3), (0.0, 1.0, 0.0, 2)]
    # query 1: refused by list 1
    recs[0, 1, :1] = [(0.5, 0.5, 0.0, 1)]
    recs[1, 1, :] = (np.nan, 0.0, 0.0, -2)
    out_ids = np.full((2, 6), -7, np.int64)
    out_sc = np.full((2, 6), 123.0, np.float32)
    ids, sc = rm.merge_rerank(recs, 4, 6, 0.5, 0.0, out_ids, out_sc)
    # candidates (cut at 4 of 5, inside the +-0 tie: id 2 before id 4): 9 (NaN), 3, 7, 2 -> adj NaN, .5, .5, .5 -> numbers, NaN last
    assert ids[0].tolist() == [3, 7, 2, 9, -7, -7]
    assert np.array_equal(sc[0], np.array([0.5, 0.5, 0.5, np.nan, 123.0, 123.0], np.float32), equal_nan=True)
    assert ids[1].tolist() == [-1] * 6 and np.isnan(sc[1]).all()
    # k below the NaN count: NaN counts as the largest value, so only NaN scores come back
    recs2 = np.zeros((1, 1, 4), rm.RECORD)
    recs2[0, 0] = [(0.9, np.nan, 0.0, 5), (0.8, np.nan, 0.0, 1), (0.7, 0.1, 0.0, 2), (0.6, np.nan, 0.0, 3)]
    ids, sc = rm.merge_rerank(recs2, 4, 2, 0.5, 0.0)
    assert ids[0].tolist() == [5, 1] and np.isnan(sc[0]).all()
    # 0 * inf: eta = 0 with an infinite dewi value
    recs2[0, 0] = [(0.9, np.inf, 0.0, 5), (0.8, 0.0, 0.0, 1), (0.7, 0.1, 0.0, 2), (0.6, -np.inf, 0.0, 3)]
    ids, sc = rm.merge_rerank(recs2, 4, 3, 0.0, 0.0)
    assert ids[0].tolist() == [1, 5, 3] and np.array_equal(sc[0], np.array([0.8, np.nan, np.nan], np.float32), equal_nan=True)

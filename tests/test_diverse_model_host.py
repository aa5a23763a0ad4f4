"""The NumPy model of the diverse (MMR) re-rank (tests/diverse_model.py) against a naive loop on hand-made cases (no GPU):
the model is what the device tests compare with, so it is checked here on its own."""
import math

import numpy as np
import pytest

import diverse_model as dm
from rerank_model import RECORD, ord32, rerank_one

F = np.float32
INF = float("inf")


def recs_of(rows):
    """[(sim, dewi, ent, id)] -> flat record array"""
    return np.array(rows, dtype=RECORD)


def naive(recs, rows, k, eta, pref, lam, max_sim=INF, id_offset=0):
    """The contract, one scalar operation at a time."""
    n_rows = len(rows)
    cand = [r for r in recs if r["id"] >= 0 and 0 <= int(r["id"]) - id_offset < n_rows]
    adj = []
    for r in cand:
        with np.errstate(invalid="ignore", over="ignore"):
            a = F(F(1.0 - eta) * r["sim"]) + F(F(eta) * r["dewi"])
            if pref != 0:
                a = F(a + F(F(pref) * r["ent"]))
        adj.append(F(a))
    n = len(cand)
    picked, order, ms = [False] * n, [], []
    lam32, oml32, cut = F(lam), F(1.0 - lam), F(max_sim)
    while len(order) < min(k, n):
        best, best_key, best_m = -1, None, None
        for t in range(n):
            if picked[t]:
                continue
            pen = None
            for s in order:
                with np.errstate(invalid="ignore", over="ignore"):
                    g = F(0)
                    acc = 0.0
                    for a, b in zip(rows[int(cand[t]["id"]) - id_offset], rows[int(cand[s]["id"]) - id_offset]):
                        acc += float(a) * float(b)
                    g = F(acc)
                if not math.isnan(g) and (pen is None or g > pen):
                    pen = g
            with np.errstate(invalid="ignore", over="ignore"):
                m = F(lam32 * adj[t])
                if pen is not None:
                    if cut != INF and pen >= cut:
                        continue
                    m = F(m - F(oml32 * pen))
            key = int(ord32(np.array([m]))[0])
            if best_key is None or key > best_key:            # strictly greater: ties stay with the lower t
                best, best_key, best_m = t, key, m
        if best < 0:
            break
        picked[best] = True
        order.append(best)
        ms.append(best_m)
    num = [j for j in range(len(order)) if not math.isnan(ms[j])]
    nan = [j for j in range(len(order)) if math.isnan(ms[j])]
    out = num + nan
    return ([int(cand[order[j]]["id"]) for j in out], [F(adj[order[j]] + F(0)) for j in out], [ms[j] for j in out])


def same(a, b):
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.where(np.isnan(a), F(0), a).view(np.uint32), np.where(np.isnan(b), F(0), b).view(np.uint32))


def check(recs, rows, k, eta, pref, lam, max_sim=INF, id_offset=0):
    rows = np.asarray(rows, dtype=F)
    ids, scores, mmr = dm.diverse_one(recs, rows, k, eta, pref, lam, max_sim, id_offset)
    n_ids, n_scores, n_mmr = naive(recs, rows, k, eta, pref, lam, max_sim, id_offset)
    assert ids.tolist() == n_ids
    assert same(scores, n_scores) and same(mmr, n_mmr)
    return ids.tolist(), scores, mmr


# unit rows with inner products that are exact in any order: e_i, and mixtures with 0.5 entries
E = np.eye(8, dtype=F)
ROWS = np.stack([E[0], E[0], E[1], (E[0] + E[1] + E[2] + E[3]) * F(0.5), E[2], E[3], np.full(8, np.nan, F), E[4]])


def test_ties_go_to_the_lower_t():
    recs = recs_of([(0.5, 0.0, 0.0, 2), (0.5, 0.0, 0.0, 4), (0.5, 0.0, 0.0, 5)])
    ids, _, _ = check(recs, ROWS, 3, 0.0, 0.0, 0.5)
    assert ids == [2, 4, 5]            # orthogonal rows: pen = 0 for all, equal m, order of t


def test_duplicate_is_pushed_back_and_pen_is_the_maximum():
    recs = recs_of([(0.9, 0.0, 0.0, 0), (0.9, 0.0, 0.0, 1), (0.6, 0.0, 0.0, 3), (0.5, 0.0, 0.0, 2)])
    ids, scores, mmr = check(recs, ROWS, 4, 0.0, 0.0, 0.5)
    # 0 first; then 1 has pen 1 (m = 0.45 - 0.5), 3 has pen 0.5 (m = 0.3 - 0.25), 2 has pen 0 (m = 0.25)
    assert ids[:2] == [0, 2]
    assert ids[2:] == [3, 1]
    assert scores.tolist() == [F(0.9), F(0.5), F(0.6), F(0.9)]


def test_nan_adj_is_picked_first_and_emitted_last():
    recs = recs_of([(0.9, 0.0, 0.0, 2), (0.8, np.nan, 0.0, 4), (0.7, 0.0, 0.0, 5)])
    ids, scores, mmr = check(recs, ROWS, 2, 0.5, 0.0, 0.5)
    assert ids == [2, 4] and np.isnan(scores[1]) and np.isnan(mmr[1])     # NaN took a place among the k, written last
    ids, _, _ = check(recs, ROWS, 3, 0.5, 0.0, 0.5)
    assert ids == [2, 5, 4]


def test_nan_rows_are_ignored_in_pen():
    recs = recs_of([(0.9, 0.0, 0.0, 6), (0.8, 0.0, 0.0, 0), (0.7, 0.0, 0.0, 1)])
    ids, _, mmr = check(recs, ROWS, 3, 0.0, 0.0, 0.5)
    assert ids == [6, 0, 1]
    assert mmr[1] == F(0.4)            # picked after the NaN row only: no number yet, m = lambda * adj
    assert mmr[2] == F(F(0.5) * F(0.7)) - F(0.5)


def test_zero_times_inf():
    recs = recs_of([(INF, 0.0, 0.0, 2), (0.5, 0.0, 0.0, 4), (-INF, 0.0, 0.0, 5)])
    ids, scores, mmr = check(recs, ROWS, 3, 0.0, 0.0, 0.0)       # lambda = 0: 0 * inf = NaN
    assert np.isnan(mmr[-1]) and np.isnan(mmr[-2])
    assert ids == [4, 2, 5] and scores.tolist() == [F(0.5), INF, -INF]
    check(recs, ROWS, 3, 1.0, 0.0, 0.5)                          # eta = 1: 0 * inf in the blend


def test_padding_and_out_of_range_ids():
    recs = recs_of([(0.9, 0.0, 0.0, 1002), (0.8, 0.0, 0.0, 5), (0.7, 0.0, 0.0, 1004), (0.6, 0.0, 0.0, 1008),
                    (-INF, 0.0, 0.0, -1), (-INF, 0.0, 0.0, -1)])
    ids, _, _ = check(recs, ROWS, 4, 0.0, 0.0, 0.5, id_offset=1000)
    assert ids == [1002, 1004]         # id 5 lies below the offset, 1008 beyond the rows: both skipped, kk = 2 < k
    out = dm.diverse_rerank(recs[None, :], ROWS, 4, 0.0, 0.0, 0.5, id_offset=1000)
    assert out[0].tolist() == [[1002, 1004, -1, -1]] and np.isnan(out[1][0, 2:]).all() and out[3].tolist() == [2]


def test_max_sim_shortens_the_result():
    recs = recs_of([(0.9, 0.0, 0.0, 0), (0.85, 0.0, 0.0, 1), (0.8, 0.0, 0.0, 3), (0.7, 0.0, 0.0, 2), (0.6, 0.0, 0.0, 4)])
    ids, _, _ = check(recs, ROWS, 5, 0.0, 0.0, 1.0, max_sim=0.9)
    assert ids == [0, 3, 2, 4]         # the copy of row 0 is struck out; lambda = 1 keeps the plain order
    ids, _, _ = check(recs, ROWS, 5, 0.0, 0.0, 1.0, max_sim=0.5)
    assert ids == [0, 2, 4]            # pen == max_sim strikes out as well (>=): row 3 goes too
    ids, _, _ = check(recs, ROWS, 5, 0.0, 0.0, 1.0, max_sim=-1.0)
    assert ids == [0]                  # everything has a number after the first pick


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_lambda_extremes_and_random_cases(lam):
    rng = np.random.RandomState(7)
    vals = np.array([0.0, -0.0, 0.25, 0.25, 0.5, -0.5, 1.0, INF, -INF, np.nan], dtype=F)
    for trial in range(40):
        c = rng.randint(1, 9)
        ids = rng.randint(0, ROWS.shape[0], size=c)
        recs = recs_of([(vals[rng.randint(len(vals))], vals[rng.randint(len(vals))], vals[rng.randint(len(vals))], i)
                        for i in ids])
        k = rng.randint(1, c + 1)
        check(recs, ROWS, k, 0.3, [0.0, 0.2][trial % 2], lam, [INF, 0.9, 0.5][trial % 3])


def test_lambda_one_is_the_plain_rerank():
    rng = np.random.RandomState(11)
    rows = rng.randn(64, 16).astype(F)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    for trial in range(30):
        c = rng.randint(1, 33)
        ids = rng.permutation(64)[:c]
        sim = np.sort(rng.choice(np.array([0.1, 0.2, 0.2, 0.7, -0.0, 0.0, np.nan, INF], dtype=F), size=c))
        recs = np.zeros(c + 3, dtype=RECORD)
        recs["id"] = -1
        recs["sim"] = -INF
        recs["sim"][:c], recs["id"][:c] = sim, ids
        recs["dewi"][:c] = rng.choice(np.array([0.0, 0.5, 0.5, np.nan, -1.0], dtype=F), size=c)
        recs["ent"][:c] = rng.rand(c).astype(F)
        # dewi_knn_candidates' order: (ord(sim) desc, id asc), the padding at the tail
        order = np.lexsort((recs["id"][:c].astype(np.int64), -ord32(recs["sim"][:c]).astype(np.int64)))
        recs[:c] = recs[:c][order]
        k = rng.randint(1, c + 1)
        pref = [0.0, 0.1][trial % 2]
        ids_m, scores_m, mmr = dm.diverse_one(recs, rows, k, 0.3, pref, 1.0)
        want_ids, want_scores = rerank_one(recs, c, k, 0.3, pref)
        assert ids_m.tolist() == want_ids.tolist()
        assert same(scores_m, want_scores)

"""NumPy model of the merge / re-rank stage (``dewi_merge_rerank``; steps 3-5 of the search on candidate records).

Contract, as the header states it.  ``lists`` is a structured array ``[n_lists][B][list_len]`` of ``(sim, dewi, ent, id)``
records, each list sorted by (sim desc, id asc) with its padding (id < 0) at the tail.  Per query:

* a record with id -2 anywhere makes the whole row -1 / NaN (a shard refused the query);
* the valid records (id >= 0) are ordered by (``ord(sim)`` desc, id asc), where ``ord`` puts NaN on top and -0 == +0; the first
  ``n_sel = min(n_candidates, n_valid)`` are the candidates, candidate rank t = 0 .. n_sel - 1;
* the blend is fp32 with one rounding per operation: ``fp32(1 - eta) * sim``, ``fp32(eta) * dewi``, their sum, then
  ``+ fp32(pref) * ent`` only when ``pref != 0``;
* the selected set is the first ``kk = min(k, n_sel)`` candidates in the order (``ord(adj)`` desc, t asc), NaN counting as the
  largest value (the reference's argpartition); they are emitted numbers first (adj desc, ties to the lower t), then the NaN
  ones in candidate-rank order (the reference's ``argsort(-adj)`` sorts NaN to the end);
* positions ``kk .. k - 1`` of both outputs are left as the caller passed them.

Not a test module.
"""
import numpy as np

RECORD = np.dtype([("sim", np.float32), ("dewi", np.float32), ("ent", np.float32), ("id", np.int32)])


def ord32(x):
    """csrc/common.hpp ``ord_f32``: an order-preserving uint32 of fp32 values, NaN on top, -0 == +0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = (x + np.float32(0)).view(np.uint32)                     # -0 + 0 == +0
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(x)] = np.uint32(0xFFFFFFFF)
    return key


def blend(sim, dewi, ent, eta, pref):
    """csrc/blend.hpp (DEWI_SIM_RAW): every product and sum rounded to fp32 once."""
    with np.errstate(invalid="ignore", over="ignore"):
        adj = np.float32(1.0 - eta) * sim.astype(np.float32) + np.float32(eta) * dewi.astype(np.float32)
        if pref != 0:
            adj = adj + np.float32(pref) * ent.astype(np.float32)
    return adj.astype(np.float32)


def record_order(recs):
    """Indices of the valid records of a flat record array in (ord(sim) desc, id asc) order; equal keys keep their place."""
    valid = np.nonzero(recs["id"] >= 0)[0]
    key = ord32(recs["sim"][valid]).astype(np.int64)
    return valid[np.lexsort((recs["id"][valid].astype(np.int64), -key))]


def rerank_one(recs, n_candidates, k, eta, pref):
    """One query's flat records -> (ids int64 [kk], scores fp32 [kk]), or None when the query is refused."""
    if np.any(recs["id"] == -2):
        return None
    cand = recs[record_order(recs)[:n_candidates]]
    n_sel = cand.shape[0]
    adj = blend(cand["sim"], cand["dewi"], cand["ent"], eta, pref)
    t = np.arange(n_sel)
    chosen = np.lexsort((t, -ord32(adj).astype(np.int64)))[: min(k, n_sel)]      # NaN first: it stays in the top k
    nan = np.isnan(adj[chosen])
    out = np.concatenate([chosen[~nan], chosen[nan]])                           # ... and is emitted last
    return cand["id"][out].astype(np.int64), (adj[out] + np.float32(0)).astype(np.float32)


def merge_rerank(lists, n_candidates, k, eta, pref, out_ids=None, out_scores=None):
    """``lists`` [n_lists][B][list_len] records -> (ids int64 [B][k], scores fp32 [B][k]).  ``out_ids`` / ``out_scores``:
    the arrays the results are written into (default: prefilled with -1 / NaN, as the package's callers do)."""
    lists = np.asarray(lists)
    assert lists.dtype == RECORD and lists.ndim == 3
    b = lists.shape[1]
    ids = np.full((b, k), -1, np.int64) if out_ids is None else out_ids
    scores = np.full((b, k), np.nan, np.float32) if out_scores is None else out_scores
    for q in range(b):
        got = rerank_one(lists[:, q, :].reshape(-1), n_candidates, k, eta, pref)
        if got is None:
            ids[q, :] = -1
            scores[q, :] = np.nan
            continue
        ids[q, : got[0].shape[0]] = got[0]
        scores[q, : got[1].shape[0]] = got[1]
    return ids, scores

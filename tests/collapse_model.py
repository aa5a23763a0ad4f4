"""NumPy model of the collapsed re-rank (``dewi_collapse_rerank``: at most ``per_group`` results per group).

Contract, as the header states it.  Per query:

* Input: c records ``(sim, dewi, ent, id)`` in ``dewi_knn_candidates``' layout and order, padding at the tail.
* Valid records: a record is valid iff ``id >= 0`` and ``id - id_offset`` lies in ``[0, n_rows)``; every other record is
  padding and ``labels`` is never indexed with it.  Candidate rank t is the position among the valid records.
* Labels: ``label_t = labels[id_t - id_offset]`` (int32 ``[n_rows]``).  Any int32 value is a group; a negative label means
  "ungrouped": such a record is a group of its own and is never folded.
* Blend: ``adj_t`` is the blend of step 4 of the search (``rerank_model.blend``): products rounded once, the ent term only if
  ``pref != 0``.
* Walk order: S = (``ord(adj_t)`` desc, t asc), NaN the largest value, -0 == +0.
* Keep rule: the record at position p of S is kept iff its label is negative or fewer than ``per_group`` records before p in S
  carry the same label ("before p" counts every earlier record, kept or not).
* Selected set: the first ``kk = min(k, number kept)`` kept records in S.
* Output: the selected records in S order, those whose adj is NaN moved behind the numbers in their own order; ids as in the
  record; scores = adj with -0 written as +0; hits = the number of valid records of the pool that carry the result's label (1
  for a negative label); ``kk``.  Positions ``kk .. k - 1`` are not written.

Not a test module.
"""
import numpy as np

import rerank_model as rm


def valid_records(recs, n_rows, id_offset):
    """Positions of the valid records of a flat record array, in order."""
    local = recs["id"].astype(np.int64) - int(id_offset)
    return np.nonzero((recs["id"] >= 0) & (local >= 0) & (local < int(n_rows)))[0]


def collapse_one(recs, labels, n_rows, k, per_group, eta, pref, id_offset=0):
    """One query's flat records -> (ids int64 [kk], scores fp32 [kk], hits int32 [kk], kk)."""
    labels = np.asarray(labels)
    assert labels.shape == (int(n_rows),)
    cand = recs[valid_records(recs, n_rows, id_offset)]
    n_sel = cand.shape[0]
    lab = labels[cand["id"].astype(np.int64) - int(id_offset)].astype(np.int64)
    adj = rm.blend(cand["sim"], cand["dewi"], cand["ent"], eta, pref)
    order = np.lexsort((np.arange(n_sel), -rm.ord32(adj).astype(np.int64)))       # S
    seen = {}
    kept = []
    for t in order.tolist():
        g = int(lab[t])
        if g < 0:
            kept.append(t)
            continue
        before = seen.get(g, 0)
        if before < per_group:
            kept.append(t)
        seen[g] = before + 1
    chosen = np.asarray(kept[: max(int(k), 0)], dtype=np.int64)
    nan = np.isnan(adj[chosen])
    out = np.concatenate([chosen[~nan], chosen[nan]]).astype(np.int64)
    hits = np.array([1 if lab[t] < 0 else seen[int(lab[t])] for t in out.tolist()], dtype=np.int32)
    return cand["id"][out].astype(np.int64), (adj[out] + np.float32(0)).astype(np.float32), hits, int(out.shape[0])


def collapse_rerank(recs, labels, n_rows, k, per_group, eta, pref, id_offset=0, out_ids=None, out_scores=None, out_hits=None,
                    out_counts=None):
    """``recs`` [B][c] records -> (ids int64 [B][k], scores fp32 [B][k], hits int32 [B][k], counts int32 [B]).  The ``out_*``
    arrays are what the results are written into (default: prefilled with -1 / NaN / 0 / 0, as the package's callers do)."""
    recs = np.asarray(recs)
    assert recs.dtype == rm.RECORD and recs.ndim == 2
    b = recs.shape[0]
    ids = np.full((b, k), -1, np.int64) if out_ids is None else out_ids
    scores = np.full((b, k), np.nan, np.float32) if out_scores is None else out_scores
    hits = np.zeros((b, k), np.int32) if out_hits is None else out_hits
    counts = np.zeros(b, np.int32) if out_counts is None else out_counts
    for q in range(b):
        i, s, h, kk = collapse_one(recs[q], labels, n_rows, k, per_group, eta, pref, id_offset)
        ids[q, :kk], scores[q, :kk], hits[q, :kk], counts[q] = i, s, h, kk
    return ids, scores, hits, counts

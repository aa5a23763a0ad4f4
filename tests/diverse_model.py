"""NumPy model of the diverse (MMR) re-rank (``dewi_diverse_rerank``), in the words of the header's contract.

Input per query: ``c`` candidate records in ``dewi_knn_candidates``' layout and order.  Records with id < 0 are padding at the
tail.

Padding and rank:

* A record whose ``id - id_offset`` lies outside ``[0, n_rows)`` is treated as padding; its row is never read.
* Candidate rank ``t`` is the position among the valid records, ``t = 0 .. n_sel - 1``.

Arithmetic:

1. ``adj_t = blend(sim, dewi, ent)``, exactly as ``rerank_model.blend``.  Products are rounded once; the ``ent`` term is added
   only if ``entropy_pref != 0``.
2. ``g(t, s)`` is the fp32 inner product of the stored rows of candidates ``t`` and ``s`` (a bf16 corpus is passed here already
   widened to fp32).  The model takes ``rows @ rows.T`` in float64 rounded to fp32 — the device's summation order is its own,
   so model and device agree bit for bit only on rows whose inner products are exact in any order — or the caller's ``gram=``
   ([n_rows, n_rows] or a callable ``(local_t, local_s) -> value``), used as given (float64 similarities stay float64).
3. Greedy selection over steps ``j = 0, 1, ...``:

   * ``pen_t = max over already picked s of g(t, s)``, ignoring NaN values (``np.fmax``).
   * If no picked row gave a number (including step 0): ``m_t = fp32(lambda) * adj_t``.
   * Otherwise ``m_t = fp32(lambda) * adj_t - fp32(1 - lambda) * pen_t``: two products, each rounded once, one subtraction.
   * A candidate is *ineligible* while ``pen_t`` is a number and ``pen_t >= fp32(max_sim)``.  ``max_sim = +inf`` disables the
     rule.
   * Pick the eligible unpicked candidate first in the order (``ord32(m_t)`` desc, ``t`` asc).  NaN counts as the largest value
     and -0 == +0.
   * Stop after k picks or when nothing is eligible: ``kk`` picks.

4. Output: the picks in pick order, with the picks whose ``m`` was NaN moved behind the numbers, keeping their own pick order;
   ids as in the record, scores ``adj_t`` with -0 written as +0, and ``m_t`` as it stood at the pick.  Positions ``kk .. k - 1``
   are left as the caller passed them.

With ``exact=True`` every operation of step 3 is carried out in float64 instead (the float64 model of the end-to-end tests),
and ``margins`` reports how decisive every step was.

Not a test module.
"""
import numpy as np

from rerank_model import blend, ord32


def valid_records(recs, n_rows, id_offset=0):
    """Positions of the valid records of one query's flat record array, in their order."""
    local = recs["id"].astype(np.int64) - int(id_offset)
    return np.nonzero((recs["id"] >= 0) & (local >= 0) & (local < int(n_rows)))[0]


def _gram_of(rows, gram, local):
    """[n_sel, n_sel] similarities of the candidates (local rows ``local``)."""
    if gram is None:
        sub = np.asarray(rows)[local].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            return (sub @ sub.T).astype(np.float32)
    if callable(gram):
        return gram(local)
    return np.asarray(gram)[np.ix_(local, local)]


def diverse_one(recs, rows, k, eta, pref, lam, max_sim=np.inf, id_offset=0, gram=None, n_rows=None, exact=False,
                margins=None):
    """One query's flat records -> (ids int64 [kk], scores fp32 [kk], mmr [kk]).

    ``exact``: the arithmetic of step 3 in float64 (``gram`` then usually float64 as well).  ``margins`` (a list): gets one
    ``(margin between the best and the second eligible m, smallest |pen - max_sim| over the unpicked)`` per step."""
    n_rows = int(np.asarray(rows).shape[0] if n_rows is None else n_rows)
    pos = valid_records(recs, n_rows, id_offset)
    cand = recs[pos]
    n_sel = cand.shape[0]
    local = cand["id"].astype(np.int64) - int(id_offset)
    adj = blend(cand["sim"], cand["dewi"], cand["ent"], eta, pref)
    g = _gram_of(rows, gram, local)
    ft = np.float64 if exact else np.float32
    lam_f, oml_f = ft(np.float32(lam)), ft(np.float32(1.0 - lam))
    cut = ft(np.float32(max_sim))
    cut_on = not np.isposinf(cut)
    pen = np.full(n_sel, np.nan, dtype=ft)
    picked = np.zeros(n_sel, dtype=bool)
    picks, ms = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(min(int(k), n_sel)):
            has = ~np.isnan(pen)
            m = lam_f * adj.astype(ft)
            m = np.where(has, m - oml_f * np.where(has, pen, ft(0)), m).astype(ft)
            eligible = ~picked & ~(cut_on & has & (pen >= cut))
            idx = np.nonzero(eligible)[0]
            if idx.size == 0:
                break
            if exact:
                key = np.where(np.isnan(m[idx]), np.inf, m[idx])
                order = idx[np.lexsort((idx, -key))]
            else:
                order = idx[np.lexsort((idx, -ord32(m[idx]).astype(np.int64)))]
            s = int(order[0])
            if margins is not None:
                gap = np.inf if order.size < 2 else float(abs(float(m[s]) - float(m[order[1]])))
                if np.isnan(gap):
                    gap = 0.0
                near = np.abs(pen[~picked & has].astype(np.float64) - float(cut)) if cut_on else np.zeros(0)
                margins.append((gap, float(near.min()) if near.size else np.inf))
            picked[s] = True
            picks.append(s)
            ms.append(m[s])
            pen = np.fmax(pen, g[:, s].astype(ft))
    picks = np.asarray(picks, dtype=np.int64)
    ms = np.asarray(ms, dtype=ft)
    nan = np.isnan(ms)
    out = np.concatenate([picks[~nan], picks[nan]])
    m_out = np.concatenate([ms[~nan], ms[nan]])
    return cand["id"][out].astype(np.int64), (adj[out] + np.float32(0)).astype(np.float32), m_out


def diverse_rerank(recs, rows, k, eta, pref, lam, max_sim=np.inf, id_offset=0, gram=None, n_rows=None):
    """``recs`` [B][c] records -> (ids int64 [B][k] prefilled -1, scores fp32 [B][k] prefilled NaN, mmr fp32 [B][k] prefilled
    NaN, kk int [B])."""
    recs = np.asarray(recs)
    b = recs.shape[0]
    ids = np.full((b, k), -1, np.int64)
    scores = np.full((b, k), np.nan, np.float32)
    mmr = np.full((b, k), np.nan, np.float32)
    kk = np.zeros(b, dtype=np.int64)
    for q in range(b):
        i, s, m = diverse_one(recs[q], rows, k, eta, pref, lam, max_sim, id_offset, gram, n_rows)
        kk[q] = i.shape[0]
        ids[q, : kk[q]], scores[q, : kk[q]], mmr[q, : kk[q]] = i, s, m
    return ids, scores, mmr, kk

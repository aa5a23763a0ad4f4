"""NumPy model of the search by examples (``dewi_knn_candidates_examples``, include/dewi_hip.h "Search by examples").

A request is P >= 1 positive and N >= 0 negative example vectors.  The contract, restated:

* an example is prepared as a query of the one-query search is: float64-summed norm, ONE rounding after the square root, IEEE
  division, left alone when the norm is 0 or NaN (``prepare_examples``);
* ``s_j(r)`` is the similarity the one-query search reports for (example j, row r) — the tests take it from the library's own
  ``range_search``, the float64 oracle computes it from scratch;
* ``p`` = max (``match="any"``) or min (``"all"``) over the positives, ``n`` = max over the negatives, fp32, exact;
* ``score = p`` without negatives; ``fl(p - fl(w * m))`` with ``w = fp32(negative_weight)``, ``m = n > 0 ? n : +0``
  (``"penalty"``); ``p > n ? p : fl(-fl(n * n))`` (``"best_score"``); NaN when ANY similarity of the row is NaN (``combine``);
* the cut is the c best OFFERED rows (the scanned rows less the excluded ones) by (``ord(score)`` desc, row asc), as
  ``dewi_candidate`` records with the payload pair and ``id_offset`` attached, padding behind ``min(c, rows offered)``; a
  record's ``sim`` went through the key: a NaN leaves as 0x7FFFFFFF, -0 as +0 (``records``);
* ``rerank_model.rerank_one`` on those records is the blend and the cut to k (``search``).

Not a test module.
"""
import numpy as np

from rerank_model import RECORD, ord32, rerank_one

EXAMPLES_MAX = 16


def prepare_examples(X):
    """Raw fp32 [E, dim] -> prepared fp32 [E, dim]."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = X.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt(np.sum(X.astype(np.float64) ** 2, axis=1)).astype(np.float32)     # one rounding, after the root
        for j in range(X.shape[0]):
            if norm[j] > 0:                                                                # false for 0 and for NaN
                out[j] = X[j] / norm[j]
    return out


def combine(S, n_positive, match="any", negative_rule="penalty", negative_weight=1.0):
    """Per-row similarities fp32 [P + N, n] -> combined scores fp32 [n]."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    assert 1 <= n_positive <= S.shape[0] <= EXAMPLES_MAX
    pos, neg = S[:n_positive], S[n_positive:]
    nan = np.isnan(S).any(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.fmin if match == "all" else np.fmax).reduce(pos, axis=0)
        if neg.shape[0] == 0:
            score = p.copy()
        else:
            n = np.fmax.reduce(neg, axis=0)
            if negative_rule == "penalty":
                m = np.where(n > 0, n, np.float32(0)).astype(np.float32)
                score = (p - (np.float32(negative_weight) * m).astype(np.float32)).astype(np.float32)
            else:
                assert negative_rule == "best_score"
                score = np.where(p > n, p, -((n * n).astype(np.float32))).astype(np.float32)
    score = score.astype(np.float32)
    score[nan] = np.nan
    return score


def through_key(x):
    """What a score looks like after its round trip through the 64-bit key (``key_score(make_key(s, row))``): every NaN is
    0x7FFFFFFF, -0 is +0, every other value keeps its bits."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    k = ord32(x)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(np.float32)


def records(score, rows, dewi32, ent32, c, exclude=(), id_offset=0):
    """``score[i]`` belongs to scanned row ``rows[i]`` (ascending; ``None``: every row) -> RECORD [c]."""
    rows = np.arange(score.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    offered = ~np.isin(rows, np.asarray(list(exclude), dtype=np.int64))
    r, s = rows[offered], score[offered]
    order = np.lexsort((r, -ord32(s).astype(np.int64)))[:c]
    out = np.zeros(c, dtype=RECORD)
    out["sim"], out["id"] = -np.inf, -1
    m = order.shape[0]
    out["sim"][:m] = through_key(s[order])
    out["dewi"][:m] = dewi32[r[order]]
    out["ent"][:m] = ent32[r[order]]
    out["id"][:m] = (r[order] + id_offset).astype(np.int32)
    return out


def search(score, rows, dewi32, ent32, c, k, eta, pref, exclude=(), id_offset=0):
    """-> (ids int64 [kk], adjusted scores fp32 [kk]): the records, then ``rerank_model.rerank_one``."""
    return rerank_one(records(score, rows, dewi32, ent32, c, exclude, id_offset), c, k, eta, pref)


def similarities64(E, X):
    """From scratch in float64: cosine of every stored row of ``E`` [n, dim] to every raw example of ``X`` -> [E, n]."""
    X64 = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = np.sqrt(np.sum(X64 ** 2, axis=1, keepdims=True))
        Xp = np.where(norm > 0, X64 / np.where(norm > 0, norm, 1.0), X64)
        return Xp @ np.asarray(E, dtype=np.float64).T


def combine64(S, n_positive, match="any", negative_rule="penalty", negative_weight=1.0):
    """``combine`` in float64 (the weight still rounded to fp32 first, as the contract says)."""
    S = np.asarray(S, dtype=np.float64)
    pos, neg = S[:n_positive], S[n_positive:]
    nan = np.isnan(S).any(axis=0)
    with np.errstate(invalid="ignore"):
        p = (np.fmin if match == "all" else np.fmax).reduce(pos, axis=0)
        if neg.shape[0] == 0:
            score = p.copy()
        else:
            n = np.fmax.reduce(neg, axis=0)
            if negative_rule == "penalty":
                score = p - np.float64(np.float32(negative_weight)) * np.where(n > 0, n, 0.0)
            else:
                score = np.where(p > n, p, -(n * n))
    score[nan] = np.nan
    return score

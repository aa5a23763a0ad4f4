"""NumPy model of the approximate int8 route (include/dewi_hip.h, "INT8 copy of the corpus").

Contract, as the header states it:

* ``Q(x)``: ``a = max |x_i|``; any NaN / inf element: ``scale = NaN``, every code 0; otherwise ``scale = fp32(a / 127)``;
  ``scale == 0``: every code 0; otherwise ``code_i = clamp(rint(fp32(x_i / scale)), -127, 127)`` (``rint``: half to even).
* a raw query is normalised first: float64-summed norm, one rounding to fp32 after the square root, fp32 division, left alone
  when the norm is 0 (or NaN); then ``Q``.
* score: ``D = sum code_row,i * code_q,i`` in exact integers, one int -> fp32 conversion, then two fp32 products in this
  order: ``fp32(fp32(float(D) * scale_row) * scale_q)``.
* candidates: the ``c`` best rows by (``ord(sim)`` desc, row asc) — NaN on top, -0 == +0 — as records (``rerank_model.RECORD``)
  with the row's payload pair and ``id = row + id_offset``; sims are written as the key holds them (-0 as +0, every NaN as
  0x7FFFFFFF); padding ``(sim -inf, 0, 0, id -1)`` behind ``min(c, n)``.
* rescore: for every record whose ``id - id_offset`` is a row, ``sim`` = the inner product of the stored fp32 row and the
  normalised fp32 query (here: float64, rounded to fp32 once); then the records with id >= 0 in ``record_order``, the ones with
  id < 0 behind them in their old order.
* search: ``rerank_model.rerank_one`` on the records.

Not a test module.
"""
import numpy as np

import rerank_model as rm

RECORD = rm.RECORD
KEY_NAN = np.array([0x7FFFFFFF], np.uint32).view(np.float32)[0]      # what csrc/common.hpp key_score gives back for a NaN


def quantize(x):
    """fp32 [..., dim] -> (codes int8 [..., dim], scales fp32 [...])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.max(np.abs(x), axis=-1)
    bad = ~np.isfinite(x).all(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        scale = (a / np.float32(127)).astype(np.float32)
        t = np.rint((x / scale[..., None]).astype(np.float32))
    scale[bad] = np.float32(np.nan)
    zero = bad | (scale == 0)
    t[zero] = 0
    codes = np.clip(t, -127, 127).astype(np.int8)
    return codes, scale


def normalize_query(q):
    """Raw fp32 queries [B, dim] -> the normalised fp32 queries: float64-summed norm, fp32 division, a zero (or NaN) norm
    leaves the query alone."""
    q = np.atleast_2d(np.ascontiguousarray(q, dtype=np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        norm = np.sqrt(np.sum(q.astype(np.float64) ** 2, axis=1)).astype(np.float32)
        qn = (q / np.where(norm > 0, norm, np.float32(1))[:, None]).astype(np.float32)
    return np.where((norm > 0)[:, None], qn, q)


def prepare_query(q):
    """Raw fp32 queries [B, dim] -> (codes int8 [B, dim], scales fp32 [B], normalised fp32 queries [B, dim])."""
    qn = normalize_query(q)
    codes, scales = quantize(qn)
    return codes, scales, qn


def scores(row_codes, row_scales, q_codes, q_scale):
    """int8 [n, dim], fp32 [n], int8 [dim], fp32 scalar -> fp32 [n] similarities."""
    d = row_codes.astype(np.int64) @ q_codes.astype(np.int64)
    assert np.abs(d).max(initial=0) < 2 ** 31
    with np.errstate(invalid="ignore"):
        s = d.astype(np.int32).astype(np.float32) * np.asarray(row_scales, np.float32)
        return (s * np.float32(q_scale)).astype(np.float32)


def key_sim(sim):
    """A similarity as a candidate record carries it: -0 as +0, every NaN as ``KEY_NAN``."""
    sim = (np.asarray(sim, np.float32) + np.float32(0)).astype(np.float32)
    return np.where(np.isnan(sim), KEY_NAN, sim).astype(np.float32)


def candidates(row_codes, row_scales, q_codes, q_scales, dewi32, ent32, c, id_offset=0):
    """Prepared queries (codes [B, dim], scales [B]) -> records [B, c]."""
    n = row_codes.shape[0]
    out = np.zeros((q_codes.shape[0], c), RECORD)
    out["sim"], out["id"] = -np.inf, -1
    for j in range(q_codes.shape[0]):
        sim = scores(row_codes, row_scales, q_codes[j], q_scales[j])
        order = np.lexsort((np.arange(n), -rm.ord32(sim).astype(np.int64)))[: min(c, n)]
        m = order.shape[0]
        out["sim"][j, :m] = key_sim(sim[order])
        out["dewi"][j, :m] = dewi32[order]
        out["ent"][j, :m] = ent32[order]
        out["id"][j, :m] = order + id_offset
    return out


def rescore(recs, rows, qn, id_offset=0):
    """Records [B, c], stored fp32 rows [n, dim], normalised fp32 queries [B, dim] -> the re-scored, re-sorted records."""
    n = rows.shape[0]
    out = recs.copy()
    rows64 = rows.astype(np.float64)
    for j in range(recs.shape[0]):
        r = recs[j].copy()
        local = r["id"].astype(np.int64) - id_offset
        valid = (r["id"] >= 0) & (local >= 0) & (local < n)
        with np.errstate(invalid="ignore"):
            r["sim"][valid] = (rows64[local[valid]] @ qn[j].astype(np.float64)).astype(np.float32)
        head = rm.record_order(r)
        tail = np.nonzero(r["id"] < 0)[0]
        out[j] = r[np.concatenate([head, tail])]
    return out


def search(recs, k, eta, pref, out_ids=None, out_scores=None):
    """Records [B, c] -> (ids int64 [B, k], scores fp32 [B, k]) by ``rerank_model.rerank_one`` (n_candidates = c)."""
    b, c = recs.shape
    ids = np.full((b, k), -1, np.int64) if out_ids is None else out_ids
    sc = np.full((b, k), np.nan, np.float32) if out_scores is None else out_scores
    for j in range(b):
        got = rm.rerank_one(recs[j], c, k, eta, pref)
        ids[j, : got[0].shape[0]] = got[0]
        sc[j, : got[1].shape[0]] = got[1]
    return ids, sc

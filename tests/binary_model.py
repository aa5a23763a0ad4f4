"""NumPy model of the approximate binary route (include/dewi_hip.h, "BINARY copy of the corpus").

Contract, as the header states it:

* shapes: cosine, fp32 rows, ``dim % 128 == 0``, ``128 <= dim <= 4096``.
* codes: a row is ``dim / 32`` dwords; bit ``i % 32`` of dword ``i / 32`` is 1 iff ``x_i > 0`` — ``+0``, ``-0``, negative values
  and NaN give 0, ``+inf`` gives 1.  No scale.  A NaN or all-zero row gets the bits this rule gives it.
* query bits: the same rule on the RAW fp32 query.
* score: ``h = popcount(row XOR query)`` over the ``dim`` bits, ``s = dim - 2 h`` in exact int32,
  ``sim = fp32(float(s) / float(dim))``: one IEEE division.  For ``dim <= 4096`` distinct ``s`` give distinct ``sim`` in the
  same order.
* candidates: the ``c`` best rows by (``ord(sim)`` desc, row asc) as records (``rerank_model.RECORD``) with the row's payload
  pair and ``id = row + id_offset``; padding ``(sim -inf, 0, 0, id -1)`` behind ``min(c, n)``.
* the whole route: ``candidates`` -> ``int8_model.rescore`` (the stored fp32 rows against the normalised query) ->
  ``int8_model.search`` (``rerank_model.rerank_one``); ``binary_cut`` (``dewi._engine``) chooses ``c``.

Not a test module.
"""
import numpy as np

import int8_model as im
import rerank_model as rm

RECORD = rm.RECORD
MIN_DIM, MAX_DIM, MAX_CANDIDATES = 128, 4096, 1024
_POP16 = np.array([bin(v).count("1") for v in range(1 << 16)], np.int32)


def binarize(x):
    """fp32 [..., dim] -> uint32 [..., dim / 32]: element i in bit i % 32 of dword i / 32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    dim = x.shape[-1]
    assert dim % 32 == 0
    with np.errstate(invalid="ignore"):
        pos = (x > 0).reshape(x.shape[:-1] + (dim // 32, 32))
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (pos.astype(np.uint64) * weights).sum(axis=-1).astype(np.uint32)


def popcount(words):
    """uint32 [...] -> int32 [...]: set bits per dword (a 16-bit table, twice)."""
    w = np.asarray(words, dtype=np.uint32)
    return _POP16[w & np.uint32(0xFFFF)] + _POP16[w >> np.uint32(16)]


def score(bits_rows, bits_q, dim):
    """uint32 [n, dim / 32], uint32 [dim / 32] -> (s int32 [n], sim fp32 [n])."""
    bits_rows = np.atleast_2d(np.asarray(bits_rows, dtype=np.uint32))
    assert bits_rows.shape[1] * 32 == dim and np.asarray(bits_q).shape == (dim // 32,)
    h = popcount(bits_rows ^ np.asarray(bits_q, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.int64)
    s = (dim - 2 * h).astype(np.int32)
    return s, sim_of(s, dim)


def sim_of(s, dim):
    """``fp32(float(s) / float(dim))``: both operands are exact in fp32, NumPy's fp32 division is the IEEE one."""
    return (np.asarray(s, np.int32).astype(np.float32) / np.float32(dim)).astype(np.float32)


def candidates(bits, q_bits, dewi32, ent32, c, id_offset=0):
    """Row bits [n, dim / 32], query bits [B, dim / 32] -> records [B, c]."""
    bits = np.atleast_2d(np.asarray(bits, dtype=np.uint32))
    q_bits = np.atleast_2d(np.asarray(q_bits, dtype=np.uint32))
    n, dim = bits.shape[0], bits.shape[1] * 32
    out = np.zeros((q_bits.shape[0], c), RECORD)
    out["sim"], out["id"] = -np.inf, -1
    for j in range(q_bits.shape[0]):
        s, sim = score(bits, q_bits[j], dim)
        order = np.lexsort((np.arange(n), -s.astype(np.int64)))[: min(c, n)]
        # (the kernel orders by ord(sim): the same order, see test_binary_model_host.py)
        m = order.shape[0]
        out["sim"][j, :m] = im.key_sim(sim[order])
        out["dewi"][j, :m] = dewi32[order]
        out["ent"][j, :m] = ent32[order]
        out["id"][j, :m] = order + id_offset
    return out


def search(stored_rows, bits, q_raw, dewi32, ent32, k, eta, pref, c, rescore=True):
    """The whole route on the host: stored fp32 rows [n, dim], their bits, RAW queries [B, dim], the cut ``c`` ->
    (ids int64 [B, k], scores fp32 [B, k])."""
    q_raw = np.atleast_2d(np.ascontiguousarray(q_raw, dtype=np.float32))
    recs = candidates(bits, binarize(q_raw), dewi32, ent32, c)
    if rescore:
        recs = im.rescore(recs, stored_rows, im.normalize_query(q_raw))
    return im.search(recs, k, eta, pref)

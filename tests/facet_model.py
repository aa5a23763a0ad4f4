"""NumPy restatement of the FACETS section of include/dewi_hip.h (a plain helper module, like predicate_model.py; not a test
module): for each of P selections of rows, the histogram of a key column over ``n_bins + 2`` slots — the bins, ``other``,
``nan`` — and, with a value column, count / min / max / sum of the values per slot.

Everything here is exact integer arithmetic or a comparison, so the device result equals it bit for bit; the one exception is
the fp64 sum of fp32 values, whose order of additions is free: ``sum_bound`` is the derived tolerance against ``math.fsum``.
"""
import math

import numpy as np

KEY_I32_RANGE, KEY_I32_EDGES, KEY_F32_EDGES = 0, 1, 2
SEL_ALL, SEL_MASKS, SEL_LISTS = 0, 1, 2
VALUE_NONE, VALUE_I32, VALUE_F32 = 0, 1, 2
MAX_BINS = 1 << 20
MAX_SELECTIONS = 4096
MAX_SLOTS = 1 << 27
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def slots_of(keys, key_kind, n_bins, key_lo=0, edges=None):
    """The slot of every key: a bin in ``[0, n_bins)``, ``n_bins`` (other) or ``n_bins + 1`` (nan)."""
    keys = np.asarray(keys)
    n_bins = int(n_bins)
    if key_kind == KEY_I32_RANGE:
        assert keys.dtype == np.int32
        b = keys.astype(np.int64) - int(key_lo)                    # 64 bits: no int32 overflow
        return np.where((b >= 0) & (b < n_bins), b, n_bins).astype(np.int64)
    want = np.int32 if key_kind == KEY_I32_EDGES else np.float32
    e = np.asarray(edges)
    assert keys.dtype == want and e.dtype == want and e.shape == (n_bins + 1,)
    with np.errstate(invalid="ignore"):
        idx = np.searchsorted(e, keys, side="right").astype(np.int64)   # how many edges are <= x (a NaN key: fixed below)
        slot = idx - 1
        slot[idx == 0] = n_bins
        slot[idx == n_bins + 1] = n_bins
        slot[keys == e[-1]] = n_bins - 1                            # the last bin is closed at both ends
    if key_kind == KEY_F32_EDGES:
        slot[np.isnan(keys)] = n_bins + 1
    return slot


def selections(n_rows, sel_kind, masks=None, rows=None, lims=None):
    """The selections as P int64 row arrays, a row once per appearance; listed ids outside ``[0, n_rows)`` are skipped."""
    if sel_kind == SEL_ALL:
        return [np.arange(n_rows, dtype=np.int64)]
    if sel_kind == SEL_MASKS:
        m = np.asarray(masks).reshape(-1, n_rows)
        return [np.flatnonzero(m[p] != 0).astype(np.int64) for p in range(m.shape[0])]
    rows, lims = np.asarray(rows, dtype=np.int64), np.asarray(lims, dtype=np.int64)
    out = []
    for p in range(len(lims) - 1):
        r = rows[lims[p]: lims[p + 1]]
        out.append(r[(r >= 0) & (r < n_rows)])
    return out


def total_order_key(values):
    """fp32 -> uint32 keys ordered by the total order of the bits (-0 below +0); int32 -> the biased value."""
    v = np.asarray(values)
    u = v.view(np.uint32)
    if v.dtype == np.int32:
        return u ^ np.uint32(0x80000000)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def facet(keys, key_kind, n_bins, key_lo=0, edges=None, sel_kind=SEL_ALL, masks=None, rows=None, lims=None, values=None):
    """``dewi_facet_run``: a dict with ``counts`` int64 [P, n_bins + 2] and, with ``values`` (int32 or float32), ``vcount``
    int64, ``vmin`` / ``vmax`` of the values' type, ``vsum`` (exact int64, wrapping; or float64 by ``math.fsum``) and
    ``vabs`` (float64 sum of |x| per slot: what ``sum_bound`` scales)."""
    keys = np.asarray(keys)
    n = keys.shape[0]
    s = int(n_bins) + 2
    slot = slots_of(keys, key_kind, n_bins, key_lo, edges)
    sels = selections(n, sel_kind, masks, rows, lims)
    out = {"counts": np.zeros((len(sels), s), dtype=np.int64)}
    if values is not None:
        values = np.asarray(values)
        is_f = values.dtype == np.float32
        assert is_f or values.dtype == np.int32
        out["vcount"] = np.zeros((len(sels), s), dtype=np.int64)
        out["vmin"] = np.full((len(sels), s), np.inf if is_f else INT32_MAX, dtype=values.dtype)
        out["vmax"] = np.full((len(sels), s), -np.inf if is_f else INT32_MIN, dtype=values.dtype)
        out["vsum"] = np.zeros((len(sels), s), dtype=np.float64 if is_f else np.int64)
        out["vabs"] = np.zeros((len(sels), s), dtype=np.float64)
    for p, r in enumerate(sels):
        sl = slot[r]
        out["counts"][p] = np.bincount(sl, minlength=s)
        if values is None:
            continue
        v = values[r]
        ok = ~np.isnan(v) if is_f else np.ones(len(v), dtype=bool)
        v, sl = v[ok], sl[ok]
        if not len(v):
            continue
        order = np.lexsort((total_order_key(v), sl))               # by slot, then by the value's key
        v, sl = v[order], sl[order]
        start = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
        end = np.r_[start[1:], len(sl)]
        b = sl[start]
        out["vcount"][p, b] = end - start
        out["vmin"][p, b] = v[start]
        out["vmax"][p, b] = v[end - 1]
        if is_f:
            wide = v.astype(np.float64)
            for lo, hi, at in zip(start.tolist(), end.tolist(), b.tolist()):
                out["vsum"][p, at] = wide[lo] if hi - lo == 1 else math.fsum(wide[lo:hi].tolist())
                out["vabs"][p, at] = abs(wide[lo]) if hi - lo == 1 else math.fsum(np.abs(wide[lo:hi]).tolist())
        else:
            out["vsum"][p, b] = np.add.reduceat(v.astype(np.int64), start)
    return out


def sum_bound(vcount, vabs):
    """``|vsum - math.fsum| <= vcount * 2^-52 * sum|x|`` per slot: the widening fp32 -> fp64 is exact, fewer than ``vcount``
    additions, each off by at most ``2^-53`` of a partial sum no larger than ``sum|x|``; the factor two covers the rounding of
    ``math.fsum``'s own result and of ``vabs``."""
    return np.asarray(vcount, dtype=np.float64) * 2.0 ** -52 * np.asarray(vabs, dtype=np.float64)


def stratify(dewi, bins, selected=None):
    """``metrics.stratify_by_dewi`` of the reference over the selected documents (``None``: all): ``{(lo, hi): proportion}``,
    the denominator every selected document, inside a bin or not; the last bin closed at both ends."""
    dewi = np.asarray(dewi, dtype=np.float32)
    e = np.asarray(bins, dtype=np.float32)
    c = facet(dewi, KEY_F32_EDGES, len(e) - 1, edges=e,
              sel_kind=SEL_ALL if selected is None else SEL_LISTS,
              rows=selected, lims=None if selected is None else [0, len(selected)])["counts"][0]
    total = int(c.sum())
    keys = [(float(bins[i]), float(bins[i + 1])) for i in range(len(bins) - 1)]
    return {k: (int(c[i]) / total if total > 0 else 0.0) for i, k in enumerate(keys)}

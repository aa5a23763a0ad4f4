"""The contract of ``dewi_select_begin`` / ``dewi_select_seed`` / ``dewi_select_run`` (include/dewi_hip.h) in NumPy: greedy
DEWI-weighted subset selection over the whole corpus.  A plain helper module, like diverse_model.py.

``g`` comes from a float64 Gram rounded to fp32: the kernel's own ``g`` wherever the inner products are exact in any order
(the synthetic rows of test_hip_select.py).  ``dtype=np.float64`` runs the same rule without any fp32 rounding and records
how clearly every pick was decided: the yardstick of the gaussian cases.
"""
import numpy as np

F32 = np.float32


def ord_f32(m):
    """common.hpp ord_f32 on an fp32 array: larger key == larger float, NaN on top, -0 == +0."""
    m = np.asarray(m, F32)
    u = (m + F32(0.0)).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(m), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def unord_f32(key):
    key = np.asarray(key, np.uint32)
    u = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key)
    return u.astype(np.uint32).view(F32)


def gram_column(E, dtype=F32):
    """``s -> g(., s)``: float64 inner products of the stored rows (bf16 rows arrive widened), rounded to ``dtype``."""
    E64 = np.asarray(E, np.float64)

    def col(s):
        with np.errstate(invalid="ignore", over="ignore"):
            return (E64 @ E64[s]).astype(dtype)
    return col


class SelectState:
    """What the workspace holds between the calls."""

    def __init__(self, n_rows, mask=None, dtype=F32):
        self.n = int(n_rows)
        self.dtype = dtype
        self.pen = np.full(self.n, np.nan, dtype)
        self.owner = np.full(self.n, -1, np.int64)
        self.struck = np.zeros(self.n, bool) if mask is None else (np.asarray(mask).astype(np.uint8) == 0)
        assert self.struck.shape == (self.n,)
        self.n_picked = 0

    def copy(self):
        c = SelectState(self.n, dtype=self.dtype)
        c.pen, c.owner, c.struck, c.n_picked = self.pen.copy(), self.owner.copy(), self.struck.copy(), self.n_picked
        return c


def _cut(max_sim, dtype):
    cut = F32(max_sim)                       # the device compares against fp32(max_sim)
    return dtype(cut), bool(cut != F32(np.inf))


def _strike(st, max_sim):
    cut, on = _cut(max_sim, st.dtype)
    if on:
        with np.errstate(invalid="ignore"):
            st.struck |= ~np.isnan(st.pen) & (st.pen >= cut)


def apply_pick(st, col, s, max_sim):
    """Row s is struck out; every other row that is not: owner, pen, the strike-out by max_sim."""
    st.struck[s] = True
    live = ~st.struck
    g = col(s)
    with np.errstate(invalid="ignore"):
        takes = live & ~np.isnan(g) & (np.isnan(st.pen) | (g > st.pen))
    st.owner[takes] = s
    st.pen[takes] = g[takes]          # (= fmax(pen, g): NaN operands are ignored)
    _strike(st, max_sim)


def seed(st, col, rows, max_sim=np.inf):
    for s in rows:
        s = int(s)
        if 0 <= s < st.n:
            apply_pick(st, col, s, max_sim)


def marginal(st, rel, lam):
    """m of every row (fp32: two products rounded once each and one subtraction)."""
    t = st.dtype
    rel = np.asarray(rel, F32).astype(t)
    with np.errstate(invalid="ignore", over="ignore"):
        m = t(lam) * rel
        has = ~np.isnan(st.pen)
        m = np.where(has, m - t(1.0 - lam) * np.where(has, st.pen, t(0)), m)
    return m.astype(t)


def run(st, col, rel, budget, lam, max_sim=np.inf, id_offset=0, margin=2e-6):
    """Up to ``budget`` more picks.  Returns (rows + id_offset, gains, first undecided pick or None): a pick is DECIDED when
    its best and second-best m differ by more than ``margin`` and no live row's pen lies within ``margin`` of max_sim
    (meaningful in float64; the fp32 model ignores it)."""
    rel = np.asarray(rel, F32)
    rows, gains, undecided = [], [], None
    _strike(st, max_sim)
    cut, on = _cut(max_sim, st.dtype)
    for j in range(min(int(budget), st.n) if budget > 0 else 0):
        ok = ~st.struck & ~np.isnan(rel)
        if not ok.any():
            break
        m = marginal(st, rel, lam)
        if st.dtype is F32:
            keys = np.where(ok, ord_f32(m).astype(np.int64), -1)
            s = int(np.argmax(keys))                     # the first of the largest: row asc
            gain = unord_f32(np.uint32(keys[s]))[()]
        else:
            mm = np.where(ok, np.where(np.isnan(m), np.inf, m), -np.inf)
            s = int(np.argmax(mm))
            gain = m[s]
            second = np.partition(mm, -2)[-2] if mm.size > 1 else -np.inf
            near_cut = False
            if on:
                has = ~np.isnan(st.pen)          # (struck-out rows too: whether they WERE struck out is the question)
                near_cut = bool(has.any() and np.min(np.abs(st.pen[has] - cut)) <= margin)
            if undecided is None and (not (mm[s] - second > margin) or near_cut):
                undecided = j
        rows.append(s + id_offset)
        gains.append(gain)
        st.n_picked += 1
        apply_pick(st, col, s, max_sim)
    return np.array(rows, np.int64), np.array(gains, st.dtype), undecided


def select(E, rel, budget, lam, max_sim=np.inf, mask=None, seeds=(), id_offset=0, dtype=F32):
    """begin + seed + run in one call: (rows, gains, state, first undecided pick)."""
    col = gram_column(E, dtype)
    st = SelectState(len(E), mask, dtype)
    seed(st, col, seeds, max_sim)
    rows, gains, und = run(st, col, rel, budget, lam, max_sim, id_offset)
    return rows, gains, st, und

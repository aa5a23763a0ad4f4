"""The contract of ``dewi_select_groups_begin`` / ``dewi_select_run_grouped`` / ``dewi_select_run_blocked_grouped``
(include/dewi_hip.h, "GROUP QUOTAS") in NumPy, on tests/select_model.py's state: the greedy selection with at most q_g picks
from group g.  A plain helper module, like select_model.py; everything that is not about groups is select_model's, unchanged.

  * row i is GROUPED when 0 <= label_i < n_groups, anything else is ungrouped and free of any quota;
  * ``GroupCounts.c[g]`` counts the grouped picks of the grouped runs (seeds and ungrouped runs do not count), never falls;
  * group g is FULL when c_g >= q_g; a grouped row of a full group is struck out, its pen and owner frozen as they stand;
  * a run: select_model's start-of-run strike, then the rows of full groups; then pick by pick — select_model's choice and
    apply_pick (the pick's own group included), c_g += 1 for a grouped pick, and a group that became full struck out.
"""
import numpy as np

import select_blocked_model as sbm
import select_model as sm

F32 = np.float32


class GroupCounts:
    """The counts the workspace holds beside select_model.SelectState (zeroed by dewi_select_groups_begin)."""

    def __init__(self, n_groups):
        self.c = np.zeros(int(n_groups), np.int64)

    def copy(self):
        out = GroupCounts(len(self.c))
        out.c = self.c.copy()
        return out


def grouped(labels, n_groups):
    lab = np.asarray(labels, np.int64)
    return (lab >= 0) & (lab < int(n_groups))


def quotas(n_groups, quota=None, per_group=1):
    """q_g: ``quota[g]``, or ``per_group`` everywhere."""
    if quota is None:
        return np.full(int(n_groups), int(per_group), np.int64)
    q = np.asarray(quota, np.int64)
    assert q.shape == (int(n_groups),)
    return q


def strike_full(st, gc, labels, q):
    """Every grouped row of a full group is struck out."""
    lab = np.asarray(labels, np.int64)
    grp = grouped(lab, len(q))
    full = gc.c >= q
    st.struck |= grp & full[np.where(grp, lab, 0)]


def count_pick(st, gc, labels, q, s):
    """Steps 5 and 6 for the pick ``s`` (already applied)."""
    lab = np.asarray(labels, np.int64)
    g = int(lab[s])
    if 0 <= g < len(q):
        gc.c[g] += 1
        if gc.c[g] >= q[g]:
            st.struck |= lab == g


def run(st, gc, col, rel, budget, lam, labels, quota=None, per_group=1, max_sim=np.inf, id_offset=0):
    """Up to ``budget`` more picks.  Returns (rows + id_offset, gains, first undecided pick or None) like select_model.run:
    each pick IS a select_model.run of one pick on the state the quotas have left."""
    q = quotas(len(gc.c), quota, per_group)
    rows, gains, undecided = [], [], None
    if budget <= 0:
        return np.array(rows, np.int64), np.array(gains, st.dtype), undecided
    sm._strike(st, max_sim)
    strike_full(st, gc, labels, q)
    for j in range(min(int(budget), st.n)):
        r, g, und = sm.run(st, col, rel, 1, lam, max_sim, id_offset)
        if len(r) == 0:
            break
        if und is not None and undecided is None:
            undecided = j
        rows.append(int(r[0]))
        gains.append(g[0])
        count_pick(st, gc, labels, q, int(r[0]) - id_offset)
    return np.array(rows, np.int64), np.array(gains, st.dtype), undecided


def select(E, rel, budget, lam, labels, n_groups, quota=None, per_group=1, max_sim=np.inf, mask=None, seeds=(), id_offset=0,
           dtype=F32):
    """begin + groups_begin + seed + run in one call: (rows, gains, state, counts, first undecided pick)."""
    col = sm.gram_column(E, dtype)
    st = sm.SelectState(len(E), mask, dtype)
    gc = GroupCounts(n_groups)
    sm.seed(st, col, seeds, max_sim)
    rows, gains, und = run(st, gc, col, rel, budget, lam, labels, quota, per_group, max_sim, id_offset)
    return rows, gains, st, gc, und


def run_blocked(st, gc, col, rel, budget, lam, labels, quota=None, per_group=1, max_sim=np.inf, block=32, s_size=64, id_offset=0,
                n_rounds=None):
    """select_blocked_model.run_blocked with quotas: the round keeps the labels of the members of S and the counts; a pick that
    fills its group empties the other members of that group at once; rows of the group outside S keep their stale keys until
    the apply pass, which only makes tau conservative.  Returns (rows + id_offset, gains, rounds that made a pick)."""
    assert st.dtype is F32
    rel = np.asarray(rel, F32)
    lab = np.asarray(labels, np.int64)
    q = quotas(len(gc.c), quota, per_group)
    cut, cut_on = sm._cut(max_sim, F32)
    rows, gains, rounds = [], [], 0
    left = min(int(budget), st.n) if budget > 0 else 0
    if left:
        sm._strike(st, max_sim)
        strike_full(st, gc, lab, q)
    tried = 0
    while left > 0 and (n_rounds is None or tried < n_rounds):
        tried += 1
        ok = ~st.struck & ~np.isnan(rel)
        if not ok.any():
            break
        keys = sbm.keys_of(sm.marginal(st, rel, lam), ok)
        order = np.argsort(keys, kind="stable")[::-1]
        order = order[keys[order] != 0]
        members = order[:s_size]
        tau = keys[order[s_size]] if len(order) > s_size else np.uint64(0)
        unsafe = bool((ok & np.isnan(st.pen)).any())
        take = min(block, left, 1 if unsafe else block)
        cur = keys[members].copy()
        pen = st.pen[members].copy()
        m_lab = np.where(grouped(lab[members], len(q)), lab[members], -1)
        cnt = gc.c.copy()                            # (the round touches only the members' groups)
        picks = []
        while len(picks) < take:
            j = int(np.argmax(cur))
            if cur[j] == 0 or cur[j] <= tau:
                break
            s = int(members[j])
            picks.append(s)
            rows.append(s + id_offset)
            gains.append(sm.unord_f32(np.uint32(cur[j] >> np.uint64(32)))[()])
            cur[j] = 0
            g = col(s)[members]
            live = cur != 0
            with np.errstate(invalid="ignore"):
                takes = live & ~np.isnan(g) & (np.isnan(pen) | (g > pen))
                pen[takes] = g[takes]
                struck = live & cut_on & ~np.isnan(pen) & (pen >= cut)
            if m_lab[j] >= 0:
                cnt[m_lab[j]] += 1
                if cnt[m_lab[j]] >= q[m_lab[j]]:
                    struck |= live & (m_lab == m_lab[j])
            new = sbm.keys_of_members(members, sbm._marginal(pen, rel[members], lam))
            cur = np.where(live & ~struck, new, np.uint64(0))
        for s in picks:                              # the apply pass
            st.n_picked += 1
            sm.apply_pick(st, col, s, max_sim)
            count_pick(st, gc, lab, q, s)
        left -= len(picks)
        rounds += bool(picks)
        if not picks:
            break
    return np.array(rows, np.int64), np.array(gains, F32), rounds

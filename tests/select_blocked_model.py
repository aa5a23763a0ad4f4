"""The round rule of the BLOCKED subset selection (``dewi_select_run_blocked``, include/dewi_hip.h) on tests/select_model.py's
state: many picks per corpus pass, bit for bit the one-pick greedy.  A plain helper module, like select_model.py.

A round, at a state whose keys are all current:
  * S = the ``s_size`` eligible rows with the largest keys ``ord(m) << 32 | ~row``; tau = the largest key of an eligible row
    outside S (0: none);
  * UNSAFE rows — eligible, pen still NaN — cap the round at ONE pick (their first number may be negative: m rises);
  * the greedy inside S: the best up-to-date key of S is the pick while it is above tau; only the members are updated, against
    the round's own picks; stop at key <= tau, S exhausted, ``block`` picks, or the budget;
  * then the picks are applied to the whole state, in pick order (``select_model.apply_pick``: the corpus pass).
"""
import numpy as np

import select_model as sm

F32 = np.float32


def keys_of(m, ok):
    """uint64 keys of the rows where ``ok``; 0 (the empty key) elsewhere."""
    row = np.arange(len(m), dtype=np.uint64)
    k = (sm.ord_f32(m).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - row)
    return np.where(ok, k, np.uint64(0))


def _marginal(pen, rel, lam):
    """select_model.marginal for given pen / rel columns (fp32)."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = F32(lam) * rel
        has = ~np.isnan(pen)
        m = np.where(has, m - F32(1.0 - lam) * np.where(has, pen, F32(0)), m)
    return m.astype(F32)


def run_blocked(st, col, rel, budget, lam, max_sim=np.inf, block=32, s_size=64, id_offset=0, n_rounds=None, unsafe_rule=True):
    """Up to ``budget`` more picks on ``st`` (fp32 state) in rounds of up to ``block`` picks; at most ``n_rounds`` rounds
    (None: until finished).  Returns (rows + id_offset, gains, rounds that made a pick).  ``unsafe_rule=False`` drops the
    one-pick cap while unsafe rows exist: NOT exact, for showing that the rule is needed."""
    assert st.dtype is F32
    rel = np.asarray(rel, F32)
    cut, cut_on = sm._cut(max_sim, F32)
    rows, gains, rounds = [], [], 0
    sm._strike(st, max_sim)
    left = min(int(budget), st.n) if budget > 0 else 0
    tried = 0
    while left > 0 and (n_rounds is None or tried < n_rounds):
        tried += 1
        ok = ~st.struck & ~np.isnan(rel)
        if not ok.any():
            break
        keys = keys_of(sm.marginal(st, rel, lam), ok)
        order = np.argsort(keys, kind="stable")[::-1]
        order = order[keys[order] != 0]
        members = order[:s_size]
        tau = keys[order[s_size]] if len(order) > s_size else np.uint64(0)
        unsafe = bool((ok & np.isnan(st.pen)).any())
        take = min(block, left, 1 if (unsafe and unsafe_rule) else block)
        cur = keys[members].copy()                 # the members' up-to-date keys; 0: picked or struck out
        pen = st.pen[members].copy()
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
            new = keys_of_members(members, _marginal(pen, rel[members], lam))
            cur = np.where(live & ~struck, new, np.uint64(0))
        for s in picks:                              # the apply pass
            st.n_picked += 1
            sm.apply_pick(st, col, s, max_sim)
        left -= len(picks)
        rounds += bool(picks)
        if not picks:
            break
    return np.array(rows, np.int64), np.array(gains, F32), rounds


def keys_of_members(members, m):
    return (sm.ord_f32(m).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - members.astype(np.uint64))

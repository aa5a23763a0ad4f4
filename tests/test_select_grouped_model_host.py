"""Group quotas of the subset selection, the model alone (no GPU): tests/select_grouped_model.py against tests/select_model.py —
the three equivalences of the contract (include/dewi_hip.h, "GROUP QUOTAS"), a hand-worked example, resume, a smaller quota on
the second run, quota 0, and the blocked round rule with quotas against the one-pick greedy."""
import itertools

import numpy as np
import pytest

import select_grouped_model as sgm
import select_model as sm
import test_hip_select_blocked as thb

INF = float("inf")
LAMS = thb.LAMS
MAX_SIMS = thb.MAX_SIMS


def col_of(gram):
    return lambda s: gram[:, s]


def same_state(a, b):
    return (np.array_equal(a.pen.view(np.uint32), b.pen.view(np.uint32)) and np.array_equal(a.owner, b.owner)
            and np.array_equal(a.struck, b.struck) and a.n_picked == b.n_picked)


def same_run(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(np.asarray(a[1], np.float32).view(np.uint32),
                                                         np.asarray(b[1], np.float32).view(np.uint32))


def plain(gram, rel, budget, lam, max_sim):
    st = sm.SelectState(len(rel))
    r, g, _ = sm.run(st, col_of(gram), rel, budget, lam, max_sim)
    return (r, g), st


def grouped(gram, rel, budget, lam, max_sim, labels, n_groups, quota=None, per_group=1):
    st, gc = sm.SelectState(len(rel)), sgm.GroupCounts(n_groups)
    r, g, _ = sgm.run(st, gc, col_of(gram), rel, budget, lam, labels, quota, per_group, max_sim)
    return (r, g), st, gc


@pytest.mark.parametrize("name", ["synthetic_200x64", "synthetic_clean_97x50", "gaussian_240x32", "antipodal_80x40"])
def test_the_three_equivalences(name):
    gram, rel = thb.cpu_corpora()[name]
    n = len(rel)
    rows = np.arange(n)
    for lam, max_sim, budget in itertools.product(LAMS, MAX_SIMS, (17, n + 3)):
        want, st = plain(gram, rel, budget, lam, max_sim)
        what = f"{name} lambda {lam} max_sim {max_sim} budget {budget}"
        # every row ungrouped: negative, n_groups and 2^31 - 1
        free = np.where(rows % 3 == 0, -1, np.where(rows % 3 == 1, 5, 0x7FFFFFFF))
        got, st2, gc = grouped(gram, rel, budget, lam, max_sim, free, 5, per_group=1)
        assert same_run(got, want) and same_state(st, st2) and not gc.c.any(), what
        # no quota can bind
        got, st2, gc = grouped(gram, rel, budget, lam, max_sim, rows % 7, 7, per_group=budget)
        assert same_run(got, want) and same_state(st, st2) and gc.c.sum() == len(want[0]), what
        # every row a group of its own, one pick each
        got, st2, gc = grouped(gram, rel, budget, lam, max_sim, rows, n, per_group=1)
        assert same_run(got, want) and same_state(st, st2) and gc.c.sum() == len(want[0]) and gc.c.max() <= 1, what


@pytest.mark.parametrize("q", [1, 3, 1000])
def test_one_group_of_all_rows_makes_min_q_eligible_picks(q):
    gram, rel = thb.cpu_corpora()["synthetic_200x64"]
    n = len(rel)
    for lam, max_sim in itertools.product(LAMS, MAX_SIMS):
        want, _ = plain(gram, rel, n + 3, lam, max_sim)
        got, st, gc = grouped(gram, rel, n + 3, lam, max_sim, np.zeros(n, np.int64), 1, per_group=q)
        k = min(q, len(want[0]))
        assert len(got[0]) == k == gc.c[0] and np.array_equal(got[0], want[0][:k])
        if k == q:
            assert st.struck.all()                     # the group is full: every row of it is struck out


def test_a_hand_worked_example_of_six_rows():
    """Orthogonal rows but for three overlaps; lambda 0.5, so m = rel / 2 - pen / 2.  Groups {0, 1, 2}, {3, 4}; row 5 is free.
    Pick 1 is row 0 (m 0.45): it gives row 1 pen 0.5, fills group 0, and rows 1 and 2 are frozen — row 1 at pen 0.5 / owner 0
    although the next pick, row 3, is 0.75 similar to it.  Pick 2 is row 3 (m 0.3): row 4 gets pen 0.25 / owner 3 and is
    frozen with group 1.  Pick 3 is row 5, the only row left; the fourth pick of the budget finds nothing."""
    gram = np.eye(6, dtype=np.float32)
    for i, j, v in [(0, 1, 0.5), (1, 3, 0.75), (3, 4, 0.25)]:
        gram[i, j] = gram[j, i] = v
    rel = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], np.float32)
    labels = np.array([0, 0, 0, 1, 1, -1])
    (rows, gains), st, gc = grouped(gram, rel, 4, 0.5, INF, labels, 2, per_group=1)
    assert rows.tolist() == [0, 3, 5]
    assert gains.tolist() == [np.float32(0.45), np.float32(0.3), np.float32(0.2)]
    assert gc.c.tolist() == [1, 1] and st.n_picked == 3 and st.struck.all()
    assert np.isnan(st.pen[0]) and st.pen[1:].tolist() == [0.5, 0.0, 0.0, 0.25, 0.0]
    assert st.owner.tolist() == [-1, 0, 0, 0, 3, 0]
    # the ungrouped run takes row 2 of group 0 next
    (rows, _), _ = plain(gram, rel, 4, 0.5, INF)
    assert rows.tolist() == [0, 2, 3, 5]


def test_resume_and_a_smaller_quota_on_the_second_run():
    gram, rel = thb.cpu_corpora()["gaussian_240x32"]
    n = len(rel)
    labels = np.where(np.arange(n) % 13 == 0, -1, np.arange(n) % 11)
    col = col_of(gram)
    for lam, max_sim in itertools.product(LAMS, MAX_SIMS):
        whole, st, gc = grouped(gram, rel, 40, lam, max_sim, labels, 11, per_group=3)
        st2, gc2 = sm.SelectState(n), sgm.GroupCounts(11)
        a = sgm.run(st2, gc2, col, rel, 15, lam, labels, None, 3, max_sim)
        b = sgm.run(st2, gc2, col, rel, 25, lam, labels, None, 3, max_sim)
        assert same_run((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), whole)
        assert same_state(st, st2) and np.array_equal(gc.c, gc2.c)
    # a second run under smaller quotas begins by striking out the groups that are full NOW
    st, gc = sm.SelectState(n), sgm.GroupCounts(11)
    first = sgm.run(st, gc, col, rel, 12, 0.5, labels, None, 3, INF)
    full_now = np.flatnonzero(gc.c >= 1)
    assert 0 < len(full_now) < 11
    second = sgm.run(st, gc, col, rel, 30, 0.5, labels, None, 1, INF)
    picked = labels[second[0]]
    assert not np.isin(picked[picked >= 0], full_now).any()
    assert (gc.c[np.setdiff1d(np.arange(11), full_now)] <= 1).all() and len(first[0]) == 12
    assert st.struck[(labels >= 0)].all() or len(second[0]) == 30


def test_quota_zero_and_negative():
    gram, rel = thb.cpu_corpora()["synthetic_clean_200x64"]
    n = len(rel)
    labels = np.arange(n) % 5
    quota = np.array([0, -3, 2, 1000, 1])
    (rows, _), st, gc = grouped(gram, rel, n + 3, 0.5, INF, labels, 5, quota=quota)
    assert gc.c.tolist()[:3] == [0, 0, 2] and gc.c[4] == 1 and gc.c[3] == (labels == 3).sum()
    assert not np.isin(labels[rows], [0, 1]).any()
    # the rows of groups 0 and 1 were struck out before the first pick: nobody ever updated them
    assert np.isnan(st.pen[np.isin(labels, [0, 1])]).all() and (st.owner[np.isin(labels, [0, 1])] == -1).all()


@pytest.mark.parametrize("name", ["synthetic_200x64", "synthetic_97x50", "synthetic_clean_200x64", "synthetic_clean_97x50",
                                  "gaussian_240x32", "antipodal_80x40"])
def test_blocked_round_rule_with_quotas_equals_the_greedy(name):
    gram, rel = thb.cpu_corpora()[name]
    n = len(rel)
    col = col_of(gram)
    rows = np.arange(n)
    patterns = [(rows % 7, 7, None, 2), (rows // 8, n // 8 + 1, None, 1), (np.where(rows % 13 == 0, -1, rows % 3), 3, None, 5),
                (rows % 5, 5, np.array([0, -1, 3, 1000, 1]), 1), (np.zeros(n, np.int64), 1, None, 9)]
    batched = 0
    for (lam, max_sim, block), (labels, n_groups, quota, per_group) in zip(
            itertools.cycle(itertools.product(LAMS, MAX_SIMS, [2, 8, 32])), patterns * 8):
        for budget, s_size in ((n + 3, 64), (48, 8)):
            one, st1, gc1 = grouped(gram, rel, budget, lam, max_sim, labels, n_groups, quota, per_group)
            st2, gc2 = sm.SelectState(n), sgm.GroupCounts(n_groups)
            r, g, rounds = sgm.run_blocked(st2, gc2, col, rel, budget, lam, labels, quota, per_group, max_sim, block, s_size)
            what = f"{name} lambda {lam} max_sim {max_sim} block {block} budget {budget} S {s_size} groups {n_groups}"
            assert same_run((r, g), one) and same_state(st1, st2) and np.array_equal(gc1.c, gc2.c), what
            batched += rounds < len(r)
    if "synthetic_" not in name or "clean" in name:
        assert batched > 0


def test_blocked_round_rule_with_quotas_resumes():
    gram, rel = thb.cpu_corpora()["gaussian_240x32"]
    n = len(rel)
    labels = np.arange(n) % 17
    whole, st, gc = grouped(gram, rel, 60, 0.5, 0.9, labels, 17, per_group=2)
    st2, gc2 = sm.SelectState(n), sgm.GroupCounts(17)
    rows, gains = [], []
    while st2.n_picked < len(whole[0]):
        form = len(rows) % 2
        if form:
            r, g, _ = sgm.run(st2, gc2, col_of(gram), rel, 3, 0.5, labels, None, 2, 0.9)
        else:
            r, g, _ = sgm.run_blocked(st2, gc2, col_of(gram), rel, 60 - st2.n_picked, 0.5, labels, None, 2, 0.9, block=8, n_rounds=1)
        assert len(r) > 0
        rows.append(r)
        gains.append(g)
    assert same_run((np.concatenate(rows), np.concatenate(gains)), whole) and same_state(st, st2) and np.array_equal(gc.c, gc2.c)

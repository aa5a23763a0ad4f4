"""Group quotas of the subset selection on the GPU: ``dewi_select_groups_begin`` / ``dewi_select_run_grouped`` /
``dewi_select_run_blocked_grouped`` (include/dewi_hip.h, "GROUP QUOTAS") against tests/select_grouped_model.py, BIT FOR BIT:
rows, gains, the count, pen, owner, the struck-out bytes, the group counts and the unwritten tail; the one-pick form against
the blocked form on the same device; the three equivalences with the ungrouped calls device against device.  Everything the
library writes is guarded (wsguard).  Corpora: test_hip_select.py's recipe through test_hip_select_blocked.corpus (exact inner
products, copies, ties, one all-NaN row; ``clean``: no NaN row, finite rel, so that rounds take many picks).

Per (corpus, N) the label patterns x quotas are all run; the twelve (lambda, max_sim) pairs, the blocks and the budget kinds
of the blocked test are dealt out over those runs, the pairing moving with the case.
"""
import itertools

import numpy as np
import pytest

import select_grouped_model as sgm
import select_model as sm
import test_hip_select as ths
import test_hip_select_blocked as thb
import wsguard

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN_ROW = ths.NAN_ROW
LAM_CUT = list(itertools.product(thb.LAMS, thb.MAX_SIMS))
PAIRS = list(itertools.product(thb.BUDGET_KINDS, thb.BLOCKS))
LAST_STATS = [0, 0, 0]                           # [rounds, passes, finished] of the last blocked call of grouped_steps
QUOTAS = [1, 2, 5, "array"]                       # per_group, or an array with 0, negative and larger-than-group entries


# ------------------------------------------------------------------------------------------------------------ plumbing
def patterns(n, rel):
    """name -> (labels int32 [n], n_groups)"""
    r = np.arange(n)
    free = np.where(r % 3 == 0, -1, np.where(r % 3 == 1, 7, 0x7FFFFFFF))      # all ungrouped beside n_groups = 7
    nan_row = r % 4 + 1
    nan_row[NAN_ROW % n] = 0                                                   # group 0 holds the NaN row and two more
    nan_row[[0, n - 1]] = 0
    nan_rel = np.where(np.isnan(rel), 0, r % 4 + 1)                            # group 0: rel all NaN (or empty) — never fills
    out = {"mod7": (r % 7, 7), "div8": (r // 8, (n - 1) // 8 + 1), "mod3": (r % 3, 3), "free": (free, 7),
           "nan_row": (nan_row, 5), "nan_rel": (nan_rel, 5), "all": (np.zeros(n), 1)}
    return {k: (np.ascontiguousarray(v[0], dtype=np.int32), v[1]) for k, v in out.items()}


def quota_of(kind, n_groups):
    """(d_quota or None, per_group)"""
    if kind == "array":
        return np.resize(np.array([0, 3, -2, 1000, 1], np.int32), n_groups), 1
    return None, kind


def grouped_steps(E, n, rel, steps, lam, max_sim, labels, n_groups, mask=None, seeds=None, id_offset=0, pattern="0xff",
                  counts_out=True):
    """begin, groups_begin, seeds, then one call per step on ONE state in a guarded workspace of the grouped size.  A step is
    (form, budget, block, quota, per_group): form "one" / "blk" = the ungrouped dewi_select_run / _run_blocked, "gone" / "gblk" =
    the grouped ones (blocked: budget + 1 rounds, enough for one pick per round; block < 0: ONE round per call until finished).
    Returns ((rows, gain, kk, pen, owner), counts after the last grouped step or None, state bytes {pen, owner, struck})."""
    import torch
    nat, lib, dim, elem = thb.lib_and_shape(E)
    total = max(int(sum(max(s[1], 0) for s in steps)), 1)
    need = int(lib.dewi_select_grouped_workspace_bytes(n, dim, elem, n_groups, 0))
    assert need > int(lib.dewi_select_blocked_workspace_bytes(n, dim, elem, 1)) > int(lib.dewi_select_workspace_bytes(n, dim, elem)) > 0
    ws = wsguard.GuardedBuffer(need, E.device, pattern, "grouped select workspace")
    o_rows = wsguard.GuardedOutput((total,), torch.int64, E.device, label="rows")
    o_gain = wsguard.GuardedOutput((total,), torch.float32, E.device, label="gain")
    o_cnt = wsguard.GuardedOutput((1,), torch.int64, E.device, label="n_picked")
    o_pen = wsguard.GuardedOutput((n,), torch.float32, E.device, label="pen")
    o_own = wsguard.GuardedOutput((n,), torch.int64, E.device, label="owner")
    o_stats = wsguard.GuardedOutput((3,), torch.int64, E.device, label="stats")
    o_grp = wsguard.GuardedOutput((n_groups,), torch.int32, E.device, label="group counts")
    rel_d = torch.from_numpy(np.ascontiguousarray(rel)).cuda()
    lab_d = wsguard.GuardedOutput((n,), torch.int32, E.device, label="labels")         # (an input: its guards show reads only)
    lab_d.mid.copy_(torch.from_numpy(labels).cuda())
    mask_d = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda()
    stream, wsp = nat.stream_ptr(), nat.ptr(ws.view)
    nat.check(lib.dewi_select_begin(n, dim, elem, nat.ptr(mask_d) if mask_d is not None else None, wsp, need, stream))
    nat.check(lib.dewi_select_groups_begin(n, dim, elem, n_groups, wsp, need, stream))
    if seeds is not None:
        seeds_d = torch.from_numpy(np.asarray(seeds, np.int64)).cuda()
        nat.check(lib.dewi_select_seed(nat.ptr(E), elem, n, dim, nat.ptr(seeds_d), len(seeds), max_sim, wsp, need, stream))
    out = (nat.ptr(o_rows.mid), nat.ptr(o_gain.mid), nat.ptr(o_cnt.mid), nat.ptr(o_pen.mid), nat.ptr(o_own.mid), wsp, need, stream)
    head = (nat.ptr(E), elem, n, dim, nat.ptr(rel_d))
    keep = []
    grouped_ran = False

    def picked():
        return 0 if bool((o_cnt.mid.view(torch.uint8) == wsguard.SENTINEL).all()) else int(o_cnt.mid.item())

    for form, b, block, quota, per_group in steps:
        grp = ()
        if form[0] == "g":
            q_d = None if quota is None else torch.from_numpy(np.ascontiguousarray(quota, dtype=np.int32)).cuda()
            keep.append(q_d)
            grp = (nat.ptr(lab_d.mid), n_groups, nat.ptr(q_d) if q_d is not None else None, per_group,
                   nat.ptr(o_grp.mid) if counts_out else None)
            grouped_ran = grouped_ran or b > 0
        if form in ("one", "gone"):
            run = lib.dewi_select_run_grouped if grp else lib.dewi_select_run
            nat.check(run(*head, b, lam, max_sim, id_offset, *out, *grp))
            continue
        run = lib.dewi_select_run_blocked_grouped if grp else lib.dewi_select_run_blocked
        if block > 0:
            nat.check(run(*head, b, lam, max_sim, id_offset, *out, block, max(b + 1, 1), nat.ptr(o_stats.mid), *grp))
            if b > 0:
                LAST_STATS[:] = o_stats.mid.tolist()
                assert LAST_STATS[2] == 1 and LAST_STATS[0] == LAST_STATS[1]
            continue
        p0, left = picked(), b
        while left > 0:                                   # one round per call, the remaining budget each time
            nat.check(run(*head, left, lam, max_sim, id_offset, *out, -block, 1, nat.ptr(o_stats.mid), *grp))
            st = o_stats.mid.tolist()
            if st[2]:
                break
            assert st[0] == 1, "an unfinished round made no pick"
            left = b - (picked() - p0)
    torch.cuda.synchronize()
    ws.check()
    for o in (o_rows, o_gain, o_cnt, o_pen, o_own, o_stats, o_grp, lab_d):
        o.check_guards()
    assert np.array_equal(lab_d.mid.cpu().numpy(), labels), "the labels were written"
    ran = any(s[1] > 0 for s in steps)
    if ran:
        for o in (o_cnt, o_pen, o_own):
            o.check_written()
    if grouped_ran and counts_out:
        o_grp.check_written()
    got = (o_rows.mid.cpu().numpy(), o_gain.mid.cpu().numpy(), int(o_cnt.mid.cpu().numpy()[0]) if ran else 0,
           o_pen.mid.cpu().numpy(), o_own.mid.cpu().numpy())
    raw = ws.view.cpu().numpy()
    state = {k: raw[o: o + ln].copy() for k, (o, ln) in thb.state_bytes(n).items()}
    return got, (o_grp.mid.cpu().numpy().copy() if grouped_ran and counts_out else None), state


def model_steps(gram, n, rel, steps, lam, max_sim, labels, n_groups, mask=None, seeds=None, id_offset=0):
    """The same steps on the model: ((rows, gains, state), counts)."""
    col = lambda s: gram[:n, s]          # noqa: E731
    st, gc = sm.SelectState(n, mask), sgm.GroupCounts(n_groups)
    if seeds is not None:
        sm.seed(st, col, seeds, max_sim)
    rows, gains = [], []
    for form, b, _, quota, per_group in steps:
        if form[0] == "g":
            r, g, _ = sgm.run(st, gc, col, rel, b, lam, labels, quota, per_group, max_sim, id_offset)
        else:
            r, g, _ = sm.run(st, col, rel, b, lam, max_sim, id_offset)
        rows.append(r)
        gains.append(g)
    return (np.concatenate(rows), np.concatenate(gains).astype(np.float32), st), gc.c


def check(got, counts, state, want, what, id_offset=0):
    (w_rows, w_gain, st), w_counts = want
    ths.assert_equal_to_model(got, (w_rows, w_gain, st), id_offset, what)
    assert np.array_equal(state["struck"] != 0, st.struck), f"{what}: struck-out bytes"
    assert np.array_equal((state["pen"].view(np.float32) + np.float32(0)).view(np.uint32),
                          (st.pen.astype(np.float32) + np.float32(0)).view(np.uint32)), f"{what}: pen in the state"
    assert np.array_equal(state["owner"].view(np.int32), st.owner.astype(np.int32)), f"{what}: owner in the state"
    if counts is not None:
        assert np.array_equal(counts.astype(np.int64), w_counts), (what, counts[:10], w_counts[:10])


def same(a, b, what):
    wsguard.assert_bit_equal(a[0], b[0], what)
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])), f"{what}: group counts"
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), f"{what}: {k} bytes of the state"


# ------------------------------------------------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("case", range(len(thb.CASES)), ids=[f"{c}-{n}" for c, n in thb.CASES])
def test_grouped_runs_equal_the_model_in_both_forms(case):
    name, n = thb.CASES[case]
    j = case
    for clean in (False, True):
        _, E, gram, rel = thb.corpus(name, clean)
        E, rel = E[:n], rel[:n]
        bmax = thb.block_max(E)
        many = 0
        runs = list(itertools.product(patterns(n, rel).items(), QUOTAS))
        if n > 300:                                            # the long corpora: one quota per pattern, moving with the case
            runs = [r for i, r in enumerate(runs) if i % len(QUOTAS) == (i // len(QUOTAS) + case + clean) % len(QUOTAS)]
        for (pname, (labels, n_groups)), qkind in runs:
            j += 7                                             # 7 is coprime to 12 and to 20: every pairing comes round
            lam, max_sim = LAM_CUT[j % len(LAM_CUT)]
            if pname == "mod3":
                max_sim = 0.25                                 # the max_sim freeze and the group freeze inside one list
            kind, block = PAIRS[j % len(PAIRS)]
            block = min(block or bmax, bmax)
            b = thb.budget_of(kind, block, n)
            quota, per_group = quota_of(qkind, n_groups)
            what = f"{name} n {n} clean {clean} {pname} quota {qkind} budget {b} block {block} lambda {lam} max_sim {max_sim}"
            want = model_steps(gram, n, rel, [("gone", b, 0, quota, per_group)], lam, max_sim, labels, n_groups)
            one = grouped_steps(E, n, rel, [("gone", b, 0, quota, per_group)], lam, max_sim, labels, n_groups,
                                pattern=("zeros", "0xff")[j % 2], counts_out=j % 3 != 0)
            check(*one, want, "one-pick " + what)
            blk = grouped_steps(E, n, rel, [("gblk", b, block, quota, per_group)], lam, max_sim, labels, n_groups,
                                pattern=("0xff", "random")[j % 2], counts_out=j % 3 != 0)
            check(*blk, want, "blocked " + what)
            same(blk, one, what)
            many += len(want[0][0]) > 1
        assert many > 0 or n == 1


# ------------------------------------------------------------------------------------------------------------ 2. copies
@pytest.mark.parametrize("name", ["f32_64", "bf16_64", "f32_768", "bf16_768"])
def test_a_cluster_of_copies_in_one_group_larger_than_the_block(name):
    """Forty copies with the highest relevance, all of ONE group: S is full of them, quota 3 lets three in and empties the
    rest of S at once; the rows of the group outside S go with the apply pass."""
    import torch
    rows, E, _, rel = thb.corpus(name, clean=True)
    n = 300
    rows, rel = rows[:n].copy(), rel[:n].copy()
    rows[100:140] = rows[100]
    rel[100:140] = np.float32(0.875)
    rel[140:180] = np.float32(0.8125)                          # the same group, not copies: live until the group fills
    Ed = E[:n].clone()
    Ed.copy_(torch.from_numpy(rows).cuda())
    gram = thb._gram(rows)
    labels = (np.arange(n) % 5 + 1).astype(np.int32)
    labels[100:180] = 0
    batched = 0
    for (lam, max_sim), block, per_group in itertools.product([(0.5, INF), (0.9, 0.9), (1.0, INF)], (8, 32), (3, 50)):
        what = f"{name} lambda {lam} max_sim {max_sim} block {block} per_group {per_group}"
        want = model_steps(gram, n, rel, [("gone", 120, 0, None, per_group)], lam, max_sim, labels, 6)
        one = grouped_steps(Ed, n, rel, [("gone", 120, 0, None, per_group)], lam, max_sim, labels, 6)
        blk = grouped_steps(Ed, n, rel, [("gblk", 120, block, None, per_group)], lam, max_sim, labels, 6)
        check(*one, want, "one-pick " + what)
        check(*blk, want, "blocked " + what)
        same(blk, one, what)
        batched += LAST_STATS[1] < blk[0][2]
        assert want[1][0] <= per_group and (lam != 1.0 or want[1][0] == per_group)
    assert batched > 0, f"{name}: no round took more than one pick"


# ------------------------------------------------------------------------------------------------------------ 3. resume, mixing
@pytest.mark.parametrize("name", ["f32_64", "f32_768", "bf16_64", "bf16_768", "f32_50"])
def test_resume_mixed_forms_and_smaller_quotas_on_one_state(name):
    n = 300
    for clean, (lam, max_sim) in itertools.product((False, True), [(0.5, INF), (0.3, 0.9)]):
        _, E, gram, rel = thb.corpus(name, clean)
        E, rel = E[:n], rel[:n]
        labels, n_groups = patterns(n, rel)["mod7"]
        arr = np.array([4, 6, 0, 9, 2, 6, 5], np.int32)
        whole = [("gone", 60, 0, None, 6)]
        parts = [("gone", 7, 0, None, 6), ("gblk", 20, 8, None, 6), ("gone", 1, 0, None, 6), ("gblk", 32, -4, None, 6)]
        what = f"{name} clean {clean} lambda {lam} max_sim {max_sim}"
        want = model_steps(gram, n, rel, whole, lam, max_sim, labels, n_groups, seeds=[9, 2], id_offset=1000)
        a = grouped_steps(E, n, rel, whole, lam, max_sim, labels, n_groups, seeds=[9, 2], id_offset=1000)
        b = grouped_steps(E, n, rel, parts, lam, max_sim, labels, n_groups, seeds=[9, 2], id_offset=1000, pattern="random")
        check(*a, want, what, 1000)
        same(b, a, "resumed " + what)
        # grouped and plain runs, blocked and one-pick, on one state; then smaller quotas (an array; per_group 1)
        mixed = [("gone", 9, 0, None, 3), ("one", 4, 0, None, 0), ("gblk", 11, 8, None, 3), ("blk", 5, 4, None, 0),
                 ("gblk", 6, 2, arr, 1), ("gone", 5, 0, arr, 1), ("gone", 40, 0, None, 1), ("gblk", 40, 16, None, 1)]
        want = model_steps(gram, n, rel, mixed, lam, max_sim, labels, n_groups, mask=np.arange(n) % 11 != 3)
        got = grouped_steps(E, n, rel, mixed, lam, max_sim, labels, n_groups, mask=np.arange(n) % 11 != 3)
        check(*got, want, "mixed " + what)


# ------------------------------------------------------------------------------------------------------------ 4. the equivalences
@pytest.mark.parametrize("name,n", [("f32_64", 2053), ("f32_50", 300), ("f32_1000", 300), ("bf16_100", 2053), ("f32_8200", 96),
                                    ("f32_64_off1", 300), ("f32_64", 1)])
def test_the_equivalences_device_against_device(name, n):
    for clean, (lam, max_sim) in itertools.product((False, True), [(0.5, INF), (0.3, 0.9), (1.0, 0.25)]):
        _, E, _, rel = thb.corpus(name, clean)
        E, rel = E[:n], rel[:n]
        bmax = thb.block_max(E)
        b = min(n + 3, 70)
        none = np.zeros(n, np.int32)
        plain = grouped_steps(E, n, rel, [("one", b, 0, None, 0)], lam, max_sim, none, 1)
        p = patterns(n, rel)
        for what, labels, n_groups, per_group in [("ungrouped", *p["free"], 1), ("no quota binds", *p["mod7"], b),
                                                  ("label = row, one each", np.arange(n, dtype=np.int32), n, 1)]:
            for form, block in (("gone", 0), ("gblk", min(8, bmax))):
                got = grouped_steps(E, n, rel, [(form, b, block, None, per_group)], lam, max_sim, labels, n_groups, counts_out=False)
                same(got, plain, f"{name} n {n} clean {clean} lambda {lam} max_sim {max_sim}: {what} ({form})")
        # one group of all rows: min(q, eligible) picks, the tail unwritten
        for q in (1, 4):
            got, counts, state = grouped_steps(E, n, rel, [("gone", b, 0, None, q)], lam, max_sim, none, 1)
            k = min(q, plain[0][2])
            assert got[2] == k == counts[0] and np.array_equal(got[0][:k], plain[0][0][:k])
            assert (got[0][k:] == ths.SENT_I64).all() and (got[1][k:].view(np.uint32) == ths.SENT_U32).all()
            assert k < q or state["struck"].all()


# ------------------------------------------------------------------------------------------------------------ 5. the workspace
@pytest.mark.parametrize("name,n", [("f32_768", 300), ("f32_50", 2053), ("bf16_100", 300), ("f32_8200", 96)])
def test_workspace_contract(name, n):
    _, E, gram, rel = thb.corpus(name)
    E, rel = E[:n], rel[:n]
    labels, n_groups = patterns(n, rel)["div8"]
    bmax = thb.block_max(E)
    steps = [("gone", 10, 0, None, 1), ("gblk", 15, min(8, bmax), None, 1)]
    mask = np.arange(n) % 5 != 0
    for lam, max_sim in [(0.5, INF), (0.3, 0.9)]:
        base = None
        for pattern in wsguard.PATTERNS:
            got = grouped_steps(E, n, rel, steps, lam, max_sim, labels, n_groups, mask=mask, seeds=[4], pattern=pattern)
            if base is None:
                base = got
                check(*got, model_steps(gram, n, rel, steps, lam, max_sim, labels, n_groups, mask=mask, seeds=[4]), name)
            same(got, base, f"{name}: workspace prefilled with {pattern}")


def test_cached_workspace_of_the_corpus_is_guarded():
    import torch
    from dewi._engine import DeviceCorpus
    _, E, gram, rel = ths.corpus("f32_768")
    n = 300
    c = DeviceCorpus(E[:n].contiguous(), torch.from_numpy(rel[:n].copy()).cuda(), torch.zeros(n, device="cuda"), space="cosine")
    labels, n_groups = patterns(n, rel[:n])["mod7"]
    kw = dict(group_labels=torch.from_numpy(labels).cuda(), n_groups=n_groups, per_group=2, return_group_counts=True)
    c.select_subset_device(4, 0.5, 0.9)                                  # the cache holds the plain size: it must grow
    first = c.select_subset_device(16, 0.5, 0.9, return_coverage=True, **kw)
    assert wsguard.guard(c) == 1
    for pattern in wsguard.PATTERNS:
        for block in (None, 8):
            wsguard.poison(c, pattern)
            got = c.select_subset_device(16, 0.5, 0.9, return_coverage=True, picks_per_pass=block, **kw)
            torch.cuda.synchronize()
            wsguard.check(c)
            wsguard.assert_bit_equal(got, first, f"cached workspace prefilled with {pattern}, block {block}")
    plain = c.select_subset_device(16, 0.5, 0.9)                         # ... and the ungrouped call works on the larger one
    torch.cuda.synchronize()
    wsguard.check(c)
    wsguard.release(c)
    (w_rows, _, _), w_counts = model_steps(gram, n, rel[:n], [("gone", 16, 0, None, 2)], 0.5, 0.9, labels, n_groups)
    kk = int(first[2].item())
    assert kk == len(w_rows) and first[0][:kk].cpu().numpy().tolist() == w_rows.tolist()
    assert first[5].cpu().numpy().tolist() == w_counts.tolist()
    assert plain[0].cpu().numpy().tolist() == ths.model_select(gram, n, rel[:n], [16], 0.5, 0.9)[0].tolist()


# ------------------------------------------------------------------------------------------------------------ 6. gaussian rows
SEEDS_C = {(3000, 200, False, 0.9, INF): 2, (3000, 200, False, 0.9, 0.8): 2, (3000, 200, True, 0.9, INF): 2,
           (3000, 200, True, 0.9, 0.8): 2}       # (n, dim, clustered, lambda, max_sim) -> seed; every other case: seed 1
CASES_C = [(n, d, b, cl, lam, ms) for (n, d, b) in ths.SHAPES_C for cl in (False, True) for lam in (0.5, 0.9) for ms in (INF, 0.8)]


@pytest.mark.parametrize("n,dim,budget,clustered,lam,max_sim", CASES_C,
                         ids=[f"{n}x{d}-{'clustered' if cl else 'plain'}-lam{lam}-cut{ms}" for n, d, b, cl, lam, ms in CASES_C])
def test_against_the_float64_model(n, dim, budget, clustered, lam, max_sim):
    """Labels row % 97 with every 13th row ungrouped, one pick per group, in both forms."""
    import torch
    seed = SEEDS_C.get((n, dim, clustered, lam, max_sim), 1)
    x, rel = ths.gaussian_corpus(n, dim, clustered, seed)
    r = np.arange(n)
    labels = np.where(r % 13 == 0, -1, r % 97).astype(np.int32)
    w_rows, w_gains, _, gc, und = sgm.select(x, rel, budget, lam, labels, 97, None, 1, max_sim, dtype=np.float64)
    decided = len(w_rows) if und is None else und
    free = sm.select(x, rel, budget, lam, max_sim, dtype=np.float64)[0]
    changed = int((free != w_rows).sum())
    print(f"seed {seed}: the float64 model made {len(w_rows)} picks, decided {decided} before its first undecided one; "
          f"the quota changes {changed} picks")
    assert len(w_rows) == budget and 4 * decided >= 3 * budget and changed > 0    # the floor, on the model alone; not vacuous
    big = torch.zeros((n + 1, dim), dtype=torch.float32, device="cuda")
    big[1:] = torch.from_numpy(x).cuda()
    one = grouped_steps(big[1:], n, rel, [("gone", budget, 0, None, 1)], lam, max_sim, labels, 97)
    blk = grouped_steps(big[1:], n, rel, [("gblk", budget, 16, None, 1)], lam, max_sim, labels, 97)
    same(blk, one, "blocked against one-pick")
    rows, gain, kk = one[0][:3]
    assert kk == budget and rows[:decided].tolist() == w_rows[:decided].tolist()
    err = np.abs(gain[:decided].astype(np.float64) - w_gains[:decided])
    print(f"largest gain error over the decided picks: {err.max():.3g}")
    assert err.max() <= 1e-5
    if decided == budget:
        assert one[1].tolist() == gc.c.tolist()


# ------------------------------------------------------------------------------------------------------------ 7. the Python layer
def check_planted_groups(planted_idx):
    idx, x, names, label, dewi, _ = planted_idx
    lab = dict(zip(names, label.tolist()))
    dw = dict(zip(names, np.float32(dewi).tolist()))
    n = len(names)
    out = []
    for per_group, block in itertools.product((1, 2), (None, 32)):
        ids = idx.select_subset_grouped(n, groups=label, per_group=per_group, mmr_lambda=0.5, picks_per_pass=block)
        count = {}
        for d in ids:
            count[lab[d]] = count.get(lab[d], 0) + 1
        size = {g: int((label == g).sum()) for g in set(label.tolist())}
        assert count == {g: min(per_group, s) for g, s in size.items()}              # every group, exactly its quota
        if per_group == 1:                                                           # ... and its member with the highest dewi
            assert all(dw[d] == max(dw[m] for m in names if lab[m] == lab[d]) for d in ids)
        out.append(ids)
    assert out[0] == out[1] and out[2] == out[3]                                     # one-pick and blocked agree
    return out


def test_planted_groups_through_exact_index_facade_and_ivf():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    want = check_planted_groups(ths.planted(ExactIndex))
    assert check_planted_groups(ths.planted(DewiIndex, use_ann=False)) == want
    assert check_planted_groups(ths.planted(IVFIndex, nlist=16, nprobe=2)) == want


def test_quotas_seeds_filter_and_groups_of_every_kind():
    import torch
    from dewi.backends import ExactIndex
    idx, x, names, label, dewi, _ = ths.planted(ExactIndex)
    n = len(names)
    stored = idx._corpus.emb.cpu().numpy()
    rel = np.random.RandomState(5).rand(n).astype(np.float32)
    allow = np.arange(n) % 3 != 0
    site = [f"site{g}" if g % 4 else None for g in label.tolist()]                    # every fourth group is free of any quota
    dense = np.array([-1 if s is None else int(s[4:]) for s in site])
    quotas = {"site1": 3, "site2": 0, "site5": 2}
    q = np.full(int(dense.max()) + 1, 1)
    q[[1, 2, 5]] = [3, 0, 2]
    seeds = [names[i] for i in np.flatnonzero(dense == 1)[:2]] + [names[int(np.flatnonzero(dense == -1)[0])]]
    seed_rows = [names.index(s) for s in seeds]
    got = idx.select_subset_grouped(40, groups=site, quotas=quotas, mmr_lambda=0.4, max_sim=0.9, relevance=rel, filter=allow,
                                    seeds=seeds, return_gain=True, return_coverage=True, picks_per_pass=None)
    for count_seeds in (True, False):
        qq = q.copy()
        qq[1] -= 2 * count_seeds
        want = sgm.select(stored, rel, 40, 0.4, dense, len(qq), qq, 1, 0.9, mask=allow, seeds=seed_rows, dtype=np.float64)
        und = len(want[0]) if want[4] is None else want[4]
        ids = idx.select_subset_grouped(40, groups=site, quotas=quotas, mmr_lambda=0.4, max_sim=0.9, relevance=rel, filter=allow,
                                        seeds=seeds, seeds_count=count_seeds)
        assert und > 0 and ids[:und] == [names[i] for i in want[0][:und]]
        picked = dense[[names.index(d) for d in ids]]
        assert (picked == 2).sum() == 0 and (picked == 1).sum() <= qq[1] and not set(ids) & set(seeds)
        assert all(allow[names.index(d)] for d in ids)
        if count_seeds:
            assert got[0] == ids and len(got[1]) == len(ids) and len(got[2]) == len(got[3]) == n
    # the other spellings of the groups: integers, a mapping, a prepared DeviceGroups, a tensor
    base = idx.select_subset_grouped(30, groups=site, per_group=2)
    ints = np.where(dense < 0, -7, dense * 1000 + 5)
    mapping = {d: s for d, s in zip(names, site) if s is not None}
    for groups in (ints, ints.tolist(), mapping, idx.make_groups(ints), torch.from_numpy(ints).cuda()):
        assert idx.select_subset_grouped(30, groups=groups, per_group=2) == base
    assert idx.select_subset_grouped(30, groups=ints, per_group=2, quotas={2005: 0}) == \
        idx.select_subset_grouped(30, groups=site, per_group=2, quotas={"site2": 0})
    assert idx.select_subset_grouped(0, groups=site) == []
    assert idx.select_subset_grouped(25, groups=[None] * n) == idx.select_subset(25)          # nobody grouped
    with pytest.raises(KeyError):
        idx.select_subset_grouped(5, groups=site, quotas={"no such site": 1})
    with pytest.raises(ValueError, match="per_group"):
        idx.select_subset_grouped(5, groups=site, per_group=0)
    with pytest.raises(ValueError):
        idx.select_subset_grouped(5, groups=site[:-1])


def test_groups_prepared_before_remove_raise():
    from dewi.backends import ExactIndex
    import dewi_oracle as orc
    rs = np.random.RandomState(3)
    n = 40
    idx = ExactIndex(dim=16)
    idx.add_batch_columns([f"d{i}" for i in range(n)], rs.randn(n, 16).astype(np.float32), orc.synth_payload_columns(n, seed=4))
    idx.build()
    groups = idx.make_groups(np.arange(n) % 4)
    assert len(idx.select_subset_grouped(8, groups=groups, per_group=1)) == 4
    idx.remove(["d3"])
    with pytest.raises(ValueError, match="another corpus"):
        idx.select_subset_grouped(8, groups=groups, per_group=1)
    assert len(idx.select_subset_grouped(8, groups=np.arange(n - 1) % 4, per_group=1)) == 4

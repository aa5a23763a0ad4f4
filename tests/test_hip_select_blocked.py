"""The blocked subset selection: ``dewi_select_seed_blocked`` / ``dewi_select_run_blocked`` (include/dewi_hip.h, "BLOCKED
form") against the one-pick calls on the same device, against tests/select_model.py, and — on the CPU —
tests/select_blocked_model.py's round rule against select_model's greedy.

The contract is equality BIT FOR BIT: rows, gains, the count, pen, owner and the unwritten tail.  Everything the library writes
is guarded (wsguard).  Corpora are test_hip_select.py's recipe (exact inner products, copies, ties, one all-NaN row — while
it is pickable every round takes one pick) and the same rows without the NaN row and with a finite rel (rounds take many).

The corpora are test_hip_select.CORPORA and bf16 768 (the same recipe, built here: that list has no bf16 row of 768 columns).

The grid (shape x N x budget x block x lambda x max_sim) is not the full cross product: per (corpus, N) EACH variant of the
corpus runs all twenty (budget kind, block) pairs, and the twelve (lambda, max_sim) pairs are dealt out over those twenty runs
(``lam_and_cut``): each variant meets all twelve, and the pairing moves with the case and the variant, so that over the cases
a (budget kind, block) pair meets every lambda and every max_sim.  Within one variant the four exhaustion runs (N + 3) have
four different lambdas and all three max_sim.
"""
import itertools

import numpy as np
import pytest

import select_blocked_model as sbm
import select_model as sm
import test_hip_select as ths

gpu = pytest.mark.gpu
INF = float("inf")
NAN_ROW = ths.NAN_ROW
LAMS = [0.0, 0.3, 0.5, 1.0]
MAX_SIMS = [INF, 0.9, 0.25]
BLOCKS = [2, 8, 32, None]                 # None: dewi_select_block_max of the shape
BUDGET_KINDS = ["one", "block-1", "block", "block+1", "all"]      # all: N + 3 (exhaustion)
NS = [1, 7, 33, 300, 2053]
# (name, bf16, dim, rows, element offset of the view inside its buffer): test_hip_select's, and bf16 768
CORPORA = list(ths.CORPORA) + [("bf16_768", True, 768, ths.N_MAX, 3 * 768)]
_cache = {}


# ------------------------------------------------------------------------------------------------------------ CPU: the rule
def _gram(rows):
    with np.errstate(invalid="ignore"):
        return (rows.astype(np.float64) @ rows.astype(np.float64).T).astype(np.float32)


def _finite_rel(rel):
    return np.where(np.isfinite(rel), rel, np.float32(0.125)).astype(np.float32)


def cpu_corpora():
    """name -> (fp32 Gram, rel)"""
    if "cpu" in _cache:
        return _cache["cpu"]
    out = {}
    for n, dim in [(200, 64), (97, 50)]:
        rows = ths.synthetic_rows(n, dim, seed=dim)
        rs = np.random.RandomState(dim + 1)
        rel = rs.choice(ths.REL_VALUES, n)
        rel[1::8] = rel[0::8][: rel[1::8].shape[0]]
        out[f"synthetic_{n}x{dim}"] = (_gram(rows), rel)
        clean = rows.copy()
        clean[NAN_ROW] = rows[NAN_ROW + 1]
        out[f"synthetic_clean_{n}x{dim}"] = (_gram(clean), _finite_rel(rel))
    rs = np.random.RandomState(7)
    x = rs.randn(240, 32)
    x[5::10] = x[4::10] + 1e-3 * rs.randn(*x[5::10].shape)         # planted near-copies
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    out["gaussian_240x32"] = (_gram(x), rs.beta(2, 2, 240).astype(np.float32))
    out["antipodal_80x40"] = antipodal()
    _cache["cpu"] = out
    return out


def antipodal():
    """+e_k and -e_k: the first pick, +e_0, gives -e_0 — the row with the LOWEST rel — pen = -1, and its m rises above everybody's."""
    eye = np.eye(40, dtype=np.float32)
    rows = np.concatenate([eye, -eye])
    rel = np.concatenate([0.9 - 0.001 * np.arange(40), 0.1 + 0.001 * np.arange(40)]).astype(np.float32)
    return _gram(rows), rel


def _both(gram, rel, budget, lam, max_sim, block, **kw):
    n = len(rel)
    col = lambda s: gram[:, s]          # noqa: E731
    st1, st2 = sm.SelectState(n), sm.SelectState(n)
    r1, g1, _ = sm.run(st1, col, rel, budget, lam, max_sim)
    r2, g2, rounds = sbm.run_blocked(st2, col, rel, budget, lam, max_sim, block, **kw)
    return (r1, g1.astype(np.float32), st1), (r2, g2, st2), rounds


def _same(a, b):
    (r1, g1, st1), (r2, g2, st2) = a, b
    return (np.array_equal(r1, r2) and np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
            and np.array_equal(st1.pen.view(np.uint32), st2.pen.view(np.uint32)) and np.array_equal(st1.owner, st2.owner)
            and np.array_equal(st1.struck, st2.struck) and st1.n_picked == st2.n_picked)


@pytest.mark.parametrize("name", ["synthetic_200x64", "synthetic_97x50", "synthetic_clean_200x64", "synthetic_clean_97x50",
                                  "gaussian_240x32", "antipodal_80x40"])
def test_round_rule_equals_the_greedy_on_the_cpu(name):
    gram, rel = cpu_corpora()[name]
    n = len(rel)
    batched = 0
    for lam, max_sim, block in itertools.product(LAMS, MAX_SIMS, [2, 8, 32]):
        for budget, s_size in ((n + 3, 64), (48, 8)):
            one, blk, rounds = _both(gram, rel, budget, lam, max_sim, block, s_size=s_size)
            assert _same(one, blk), f"{name} lambda {lam} max_sim {max_sim} block {block} budget {budget} S {s_size}"
            batched += rounds < len(blk[0])
    if "synthetic_" not in name or "clean" in name:
        assert batched > 0          # without a live NaN row rounds take more than one pick


def test_round_rule_resumes_on_the_cpu():
    gram, rel = cpu_corpora()["gaussian_240x32"]
    n = len(rel)
    col = lambda s: gram[:, s]          # noqa: E731
    whole = sm.SelectState(n)
    want = sm.run(whole, col, rel, 100, 0.5, 0.9)
    st = sm.SelectState(n)
    rows, gains = [], []
    while st.n_picked < len(want[0]):          # one round per call, the remaining budget each time
        r, g, _ = sbm.run_blocked(st, col, rel, 100 - st.n_picked, 0.5, 0.9, block=8, n_rounds=1)
        assert len(r) > 0
        rows.append(r)
        gains.append(g)
    assert _same((want[0], want[1].astype(np.float32), whole), (np.concatenate(rows), np.concatenate(gains), st))


def test_the_unsafe_rule_is_needed():
    """Antipodal rows: after the first pick the row with the lowest rel has the largest m.  The rule (one pick per round while a
    live eligible row has no pen yet) keeps the blocked form exact; without it the first round goes on with stale keys."""
    gram, rel = antipodal()
    one, blk, _ = _both(gram, rel, 20, 0.5, INF, 8)
    assert _same(one, blk) and one[0][:2].tolist() == [0, 40]
    _, wrong, _ = _both(gram, rel, 20, 0.5, INF, 8, unsafe_rule=False)
    assert wrong[0][:2].tolist() == [0, 1]


def test_python_signature_of_the_blocked_method():
    """``select_subset`` keeps its parameter list (tests/test_select_host.py pins it): the blocked form is a method of its own."""
    import inspect
    from dewi._engine import DeviceCorpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    for cls in (ExactIndex, DewiIndex, IVFIndex):
        plain, blocked = inspect.signature(cls.select_subset), inspect.signature(cls.select_subset_blocked)
        assert list(blocked.parameters) == list(plain.parameters) + ["picks_per_pass"], cls.__name__
        assert all(blocked.parameters[k].default == v.default for k, v in plain.parameters.items())
        assert blocked.parameters["picks_per_pass"].default == 32
    assert IVFIndex.select_subset_blocked is ExactIndex.select_subset_blocked
    sig = inspect.signature(DeviceCorpus.select_subset_device)
    assert sig.parameters["picks_per_pass"].default is None and sig.parameters["return_stats"].default is False


# ------------------------------------------------------------------------------------------------------------ GPU plumbing
def corpus(name, clean=False):
    """test_hip_select.corpus (its recipe, for the one corpus that module does not have), or — ``clean`` — the same rows with
    the NaN row replaced by a copy of its neighbour and every rel finite: (host rows, device view at the same odd offset,
    fp32 Gram, rel)."""
    import torch
    if not clean and any(c[0] == name for c in ths.CORPORA):
        return ths.corpus(name)
    key = (clean, name)
    if key not in _cache:
        _, bf16, dim, n, off = next(c for c in CORPORA if c[0] == name)
        if clean:
            rows, _, _, rel = corpus(name)
            rows, rel = rows.copy(), _finite_rel(rel)
            if n > NAN_ROW:
                rows[NAN_ROW] = rows[NAN_ROW + 1]
        else:
            rows = ths.synthetic_rows(n, dim, seed=dim)
            rel = np.random.RandomState(dim + 1).choice(ths.REL_VALUES, n)
            rel[1::8] = rel[0::8][: rel[1::8].shape[0]]
        flat = torch.zeros(off + n * dim + 8, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        view = flat[off: off + n * dim].view(n, dim)
        view.copy_(torch.from_numpy(rows).cuda())          # (+-0.25, 0 and NaN are exact in bf16)
        _cache[key] = (rows, view, _gram(rows), rel, flat)
    return _cache[key][:4]


def lib_and_shape(E):
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    return nat, lib, int(E.shape[1]), 1 if E.dtype == torch.bfloat16 else 0


def block_max(E):
    _, lib, dim, elem = lib_and_shape(E)
    return int(lib.dewi_select_block_max(dim, elem))


def state_bytes(n):
    """(offset, length) of pen / owner / struck inside a workspace: DESIGN.md 3.1 (the one-pick layout, shared by both forms)."""
    n64 = (n + 63) // 64 * 64
    pen = 2 * 256 * 8 + 256
    return {"pen": (pen, 4 * n), "owner": (pen + 4 * n64, 4 * n), "struck": (pen + 8 * n64, n)}


def device_steps(E, n, rel, steps, lam, max_sim, mask=None, seeds=None, seed_block=0, id_offset=0, pattern="0xff",
                 coverage=True, want_state=False):
    """begin, seeds (``seed_block`` > 0: dewi_select_seed_blocked), then one call per step on ONE state in a workspace of the
    blocked size.  A step is (form, budget, block, n_rounds): form "one" = dewi_select_run; "blk" = dewi_select_run_blocked
    with n_rounds (None: budget + 1, enough for one pick per round); "loop" = n_rounds = 1, called until finished.  Returns
    ((rows, gain, kk, pen, owner), stats) — stats = [rounds, passes, finished of the last blocked call] summed over the calls —
    and with ``want_state`` the state's pen / owner / struck bytes."""
    import torch
    import wsguard
    nat, lib, dim, elem = lib_and_shape(E)
    bmax = int(lib.dewi_select_block_max(dim, elem))
    assert bmax >= 1
    total = max(int(sum(max(s[1], 0) for s in steps)), 1)
    need = int(lib.dewi_select_blocked_workspace_bytes(n, dim, elem, bmax))
    assert need >= int(lib.dewi_select_workspace_bytes(n, dim, elem)) > 0
    ws = wsguard.GuardedBuffer(need, E.device, pattern, "blocked select workspace")
    o_rows = wsguard.GuardedOutput((total,), torch.int64, E.device, label="rows")
    o_gain = wsguard.GuardedOutput((total,), torch.float32, E.device, label="gain")
    o_cnt = wsguard.GuardedOutput((1,), torch.int64, E.device, label="n_picked")
    o_pen = wsguard.GuardedOutput((n,), torch.float32, E.device, label="pen")
    o_own = wsguard.GuardedOutput((n,), torch.int64, E.device, label="owner")
    o_stats = wsguard.GuardedOutput((3,), torch.int64, E.device, label="stats")
    rel_d = torch.from_numpy(np.ascontiguousarray(rel)).cuda()
    mask_d = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda()
    stream = nat.stream_ptr()
    wsp = nat.ptr(ws.view)
    nat.check(lib.dewi_select_begin(n, dim, elem, nat.ptr(mask_d) if mask_d is not None else None, wsp, need, stream))
    if seeds is not None:
        seeds_d = torch.from_numpy(np.asarray(seeds, np.int64)).cuda()
        if seed_block:
            nat.check(lib.dewi_select_seed_blocked(nat.ptr(E), elem, n, dim, nat.ptr(seeds_d), len(seeds), max_sim, wsp, need, stream,
                                                   seed_block))
        else:
            nat.check(lib.dewi_select_seed(nat.ptr(E), elem, n, dim, nat.ptr(seeds_d), len(seeds), max_sim, wsp, need, stream))
    out = (nat.ptr(o_rows.mid), nat.ptr(o_gain.mid), nat.ptr(o_cnt.mid), nat.ptr(o_pen.mid) if coverage else None,
           nat.ptr(o_own.mid) if coverage else None, wsp, need, stream)
    stats = [0, 0, 0]

    def blocked(budget, block, rounds):
        nat.check(lib.dewi_select_run_blocked(nat.ptr(E), elem, n, dim, nat.ptr(rel_d), budget, lam, max_sim, id_offset, *out, block,
                                              rounds, nat.ptr(o_stats.mid)))
        if budget > 0:                                   # (a budget of 0 writes nothing)
            st = o_stats.mid.tolist()
            stats[:] = [stats[0] + st[0], stats[1] + st[1], st[2]]

    def picked():
        return 0 if bool((o_cnt.mid.view(torch.uint8) == wsguard.SENTINEL).all()) else int(o_cnt.mid.item())

    for form, b, block, n_rounds in steps:
        if form == "one":
            nat.check(lib.dewi_select_run(nat.ptr(E), elem, n, dim, nat.ptr(rel_d), b, lam, max_sim, id_offset, *out))
        elif form == "blk":
            blocked(b, block, max(b + 1, 1) if n_rounds is None else n_rounds)
        else:                                            # one round per call, the remaining budget each time
            p0, left = picked(), b
            while left > 0:
                before = stats[0]
                blocked(left, block, 1)
                if stats[2]:
                    break
                assert stats[0] == before + 1, "an unfinished round made no pick"
                left = b - (picked() - p0)
    torch.cuda.synchronize()
    ws.check()
    for o in (o_rows, o_gain, o_cnt, o_pen, o_own, o_stats):
        o.check_guards()
    if any(s[1] > 0 for s in steps):
        o_cnt.check_written()
        if coverage:
            o_pen.check_written()
            o_own.check_written()
    got = (o_rows.mid.cpu().numpy(), o_gain.mid.cpu().numpy(), int(o_cnt.mid.cpu().numpy()[0]) if any(s[1] > 0 for s in steps) else 0,
           o_pen.mid.cpu().numpy(), o_own.mid.cpu().numpy())
    if want_state:
        raw = ws.view.cpu().numpy()
        return got, stats, {k: raw[o: o + ln].copy() for k, (o, ln) in state_bytes(n).items()}
    return got, stats


def assert_same(got, base, what):
    import wsguard
    wsguard.assert_bit_equal(got, base, what)


def budget_of(kind, block, n):
    return {"one": 1, "block-1": block - 1, "block": block, "block+1": block + 1, "all": n + 3}[kind]


# ------------------------------------------------------------------------------------------------------------ 1. the grid
CASES = [(c[0], n) for c in CORPORA if c[0] != "f32_64_off1" for n in (NS if c[3] == ths.N_MAX else [c[3]])] + [("f32_64_off1", 300)]
PAIRS = list(itertools.product(BUDGET_KINDS, BLOCKS))
LAM_CUT = list(itertools.product(LAMS, MAX_SIMS))


def lam_and_cut(case, clean, j):
    """(lambda, max_sim) of run j (the j-th (budget kind, block) pair) of a variant of a case: i -> (LAMS[i % 4], MAX_SIMS[i % 3])
    is one-to-one on twelve consecutive i, and 7 is coprime to 12, so twelve consecutive j meet all twelve pairs; runs 16 .. 19
    (budget N + 3 at the four blocks) step lambda by 3 places and max_sim by one: four different lambdas, all three max_sim.
    The offset moves the pairing from case to case and between the two variants."""
    i = 7 * j + case + 5 * clean
    return LAMS[i % len(LAMS)], MAX_SIMS[i % len(MAX_SIMS)]


def test_the_grid_deals_every_pair_to_both_variants():
    for case, clean in itertools.product(range(len(CASES)), (0, 1)):
        dealt = [lam_and_cut(case, clean, j) for j in range(len(PAIRS))]
        assert set(dealt) == set(LAM_CUT)
        assert [p[0] for p in PAIRS[16:]] == ["all"] * 4
        assert len({lam for lam, _ in dealt[16:]}) == 4 and {cut for _, cut in dealt[16:]} == set(MAX_SIMS)
    for j, clean in itertools.product(range(len(PAIRS)), (0, 1)):          # over the cases a pair meets every (lambda, max_sim)
        assert {lam_and_cut(case, clean, j) for case in range(len(CASES))} == set(LAM_CUT)


@gpu
@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{c}-{n}" for c, n in CASES])
def test_blocked_equals_one_pick_and_the_model(case):
    name, n = CASES[case]
    for clean in (False, True):
        _, E, gram, rel = corpus(name, clean)
        E, rel = E[:n], rel[:n]
        bmax = block_max(E)
        many = 0
        for j, (kind, block) in enumerate(PAIRS):
            lam, max_sim = lam_and_cut(case, clean, j)
            block = min(block or bmax, bmax)                       # (f32_8200: every block is clipped to block_max)
            b = budget_of(kind, block, n)
            what = f"{name} n {n} clean {clean} budget {b} block {block} lambda {lam} max_sim {max_sim}"
            got, stats = device_steps(E, n, rel, [("blk", b, block, None)], lam, max_sim, pattern=("zeros", "0xff")[j % 2])
            base, _ = device_steps(E, n, rel, [("one", b, 0, 0)], lam, max_sim)
            assert_same(got, base, what)
            ths.assert_equal_to_model(got, ths.model_select(gram, n, rel, [b], lam, max_sim), what=what)
            if b > 0:
                assert stats[2] == 1 and stats[0] == stats[1] <= max(got[2], 0), (what, stats)
                many += stats[1] < got[2]
        if clean and n >= 33:
            assert many > 0, f"{name} n {n}: no round took more than one pick"


# ------------------------------------------------------------------------------------------------------------ 2. copies
@gpu
@pytest.mark.parametrize("name", ["f32_64", "bf16_64", "f32_768", "bf16_768"])
def test_a_cluster_of_copies_larger_than_the_block(name):
    """Rows 40 .. 59 are exact copies with the largest rel: they fill the head of S, and under max_sim = 0.9 the round's first pick
    strikes all of them out."""
    import torch
    rows, _, _, rel = corpus(name, clean=True)
    n = 300
    rows, rel = rows[:n].copy(), rel[:n].copy()
    rows[40:60] = rows[40]
    rel[40:60] = 0.875
    E = torch.from_numpy(rows).cuda().to(torch.bfloat16 if name.startswith("bf16") else torch.float32)
    gram = _gram(rows)
    for block, lam in itertools.product([8, 16], [0.5, 1.0]):
        got, stats = device_steps(E, n, rel, [("blk", 30, block, None)], lam, 0.9)
        base, _ = device_steps(E, n, rel, [("one", 30, 0, 0)], lam, 0.9)
        assert_same(got, base, f"{name} block {block} lambda {lam}")
        ths.assert_equal_to_model(got, ths.model_select(gram, n, rel, [30], lam, 0.9), what=name)
        picked = got[0][: got[2]]
        assert picked[0] == 40 and not set(range(41, 60)) & set(picked.tolist())


# ------------------------------------------------------------------------------------------------------------ 3. mask, rel, id_offset
@gpu
@pytest.mark.parametrize("name", ["f32_64", "f32_50", "f32_768", "bf16_100", "bf16_768", "f32_8200"])
def test_mask_special_rel_and_id_offset(name):
    _, E, gram, rel = corpus(name)                      # (rel holds NaN, +-inf and +-0; the NaN row is masked out below)
    n = min(300, E.shape[0])
    E, rel = E[:n], rel[:n]
    rs = np.random.RandomState(3)
    mask = rs.rand(n) < 0.6
    mask[NAN_ROW] = False
    bmax = block_max(E)
    for (lam, max_sim), block in itertools.product([(0.5, INF), (0.0, 0.9), (1.0, 0.25), (0.3, 0.9)], [2, 8, 32]):
        block = min(block, bmax)
        got, stats = device_steps(E, n, rel, [("blk", 40, block, None)], lam, max_sim, mask=mask, id_offset=1000)
        base, _ = device_steps(E, n, rel, [("one", 40, 0, 0)], lam, max_sim, mask=mask, id_offset=1000)
        what = f"{name} block {block} lambda {lam} max_sim {max_sim}"
        assert_same(got, base, what)
        ths.assert_equal_to_model(got, ths.model_select(gram, n, rel, [40], lam, max_sim, mask=mask, id_offset=1000), id_offset=1000,
                                  what=what)
        assert mask[got[0][: got[2]] - 1000].all()


# ------------------------------------------------------------------------------------------------------------ 4. seeds
@gpu
@pytest.mark.parametrize("name", ["f32_64", "f32_50", "f32_768", "bf16_64", "bf16_768", "f32_8200", "f32_64_off1"])
def test_seeds_blocked_leave_the_state_of_the_one_pick_seeds(name):
    _, E, gram, rel = corpus(name)
    n = min(300, E.shape[0])
    E, rel = E[:n], rel[:n]
    mask = np.ones(n, bool)
    mask[12] = False
    rs = np.random.RandomState(11)
    seeds = rs.randint(0, n, 41).tolist()
    seeds[3:3] = [8, 9, 8, n + 5, -1, 12, NAN_ROW, 8]          # a copy pair, a repeat, junk rows, the masked row, the NaN row
    bmax = block_max(E)
    for block, max_sim in itertools.product([2, 8, 32], [INF, 0.9, 0.25]):
        block = min(block, bmax)
        assert len(seeds) > block
        got, _, st_b = device_steps(E, n, rel, [("blk", 10, block, None)], 0.5, max_sim, mask=mask, seeds=seeds, seed_block=block,
                                    want_state=True)
        base, _, st_1 = device_steps(E, n, rel, [("one", 10, 0, 0)], 0.5, max_sim, mask=mask, seeds=seeds, want_state=True)
        what = f"{name} block {block} max_sim {max_sim}"
        assert_same(got, base, what)
        for k in st_1:
            assert np.array_equal(st_b[k], st_1[k]), f"{what}: the {k} column of the state differs"
        ths.assert_equal_to_model(got, ths.model_select(gram, n, rel, [10], 0.5, max_sim, mask=mask, seeds=seeds), what=what)
    # the state right after the seeds, before any run
    for block in (2, min(32, bmax)):
        _, _, st_b = device_steps(E, n, rel, [], 0.5, 0.9, mask=mask, seeds=seeds, seed_block=block, want_state=True, coverage=False)
        _, _, st_1 = device_steps(E, n, rel, [], 0.5, 0.9, mask=mask, seeds=seeds, want_state=True, coverage=False)
        for k in st_1:
            assert np.array_equal(st_b[k], st_1[k]), f"{name} block {block}: the {k} column after the seeds differs"


# ------------------------------------------------------------------------------------------------------------ 5. resume, mixing
@gpu
@pytest.mark.parametrize("name", ["f32_64", "f32_768", "bf16_64", "bf16_768", "f32_50"])
def test_resume_and_mixing_on_one_state(name):
    for clean in (False, True):
        _, E, gram, rel = corpus(name, clean)
        n = 300
        E, rel = E[:n], rel[:n]
        for (b1, b2, b3), lam, max_sim, block in itertools.product([(3, 9, 20), (17, 1, 40)], [0.3, 1.0], [INF, 0.9], [8]):
            b = b1 + b2 + b3
            whole_1, _ = device_steps(E, n, rel, [("one", b, 0, 0)], lam, max_sim, seeds=[2], id_offset=7)
            whole_b, _ = device_steps(E, n, rel, [("blk", b, block, None)], lam, max_sim, seeds=[2], id_offset=7)
            mixed, _ = device_steps(E, n, rel, [("blk", b1, block, None), ("one", b2, 0, 0), ("blk", b3, block, None)], lam, max_sim,
                                    seeds=[2], id_offset=7)
            looped, stats = device_steps(E, n, rel, [("loop", b, block, 1)], lam, max_sim, seeds=[2], id_offset=7)
            what = f"{name} clean {clean} {b1}+{b2}+{b3} lambda {lam} max_sim {max_sim}"
            assert_same(whole_b, whole_1, what + ": one blocked run")
            assert_same(mixed, whole_1, what + ": blocked, one-pick, blocked")
            assert_same(looped, whole_1, what + ": n_rounds = 1 until finished")
            assert stats[2] == 1
            ths.assert_equal_to_model(whole_b, ths.model_select(gram, n, rel, [b], lam, max_sim, seeds=[2], id_offset=7), id_offset=7,
                                      what=what)
            # a run that stops unfinished (2 rounds), then the remaining budget in the other form
            part, st = device_steps(E, n, rel, [("blk", b, block, 2)], lam, max_sim, seeds=[2], id_offset=7)
            assert part[2] <= 2 * block and (st[2] == 1) == (part[2] == whole_1[2])
            if part[2] < whole_1[2]:
                rest, _ = device_steps(E, n, rel, [("blk", b, block, 2), ("one", b - part[2], 0, 0)], lam, max_sim, seeds=[2], id_offset=7)
                assert (rest[0][b:] == ths.SENT_I64).all() and (rest[1][b:].view(np.uint32) == ths.SENT_U32).all()
                assert_same((rest[0][:b], rest[1][:b]) + rest[2:], whole_1, what + ": two rounds, then one-pick")


# ------------------------------------------------------------------------------------------------------------ 6, 7. gaussian rows
def gaussian(bf16, copies):
    import torch
    key = ("gauss", bf16, copies)
    if key not in _cache:
        rs = np.random.RandomState(17)
        x = rs.randn(2053, 768)
        if copies:
            x[5::10] = x[4::10][: x[5::10].shape[0]] + 1e-3 * rs.randn(*x[5::10].shape)
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        rel = rs.beta(2, 2, 2053).astype(np.float32)
        E = torch.from_numpy(x).cuda()
        _cache[key] = (E.to(torch.bfloat16) if bf16 else E, rel)
    return _cache[key]


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("copies", [False, True], ids=["plain", "copies"])
def test_gaussian_rows_bit_equal_and_really_batched(bf16, copies):
    """Ties are not exact here; both forms use one summation order, so equality holds whatever the data.  The caps on the
    passes are conditions, not measurements: S is built from PER-WORKGROUP lists (each workgroup's best 16 keys), not from a
    global top-C, so the lambda = 1 figure is the upper bound budget // 8 too (a global top-C would give exactly
    1 + ceil((budget - 1) / block))."""
    E, rel = gaussian(bf16, copies)
    n, budget, block = 2053, 512, 32
    for lam, max_sim in [(0.5, INF), (0.5, 0.9), (1.0, INF)]:
        got, stats = device_steps(E, n, rel, [("blk", budget, block, None)], lam, max_sim)
        base, _ = device_steps(E, n, rel, [("one", budget, 0, 0)], lam, max_sim)
        assert_same(got, base, f"bf16 {bf16} copies {copies} lambda {lam} max_sim {max_sim}")
        print(f"bf16 {bf16} copies {copies} lambda {lam} max_sim {max_sim}: {got[2]} picks, {stats[0]} rounds, {stats[1]} passes")
        assert got[2] == budget and stats[2] == 1
        assert stats[1] <= budget // 8, stats


# ------------------------------------------------------------------------------------------------------------ 8. the Python layer
class CountingLib:
    """The ctypes library with a count of the blocked calls made through it."""

    def __init__(self, lib):
        self._lib, self.blocked = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name in ("dewi_select_seed_blocked", "dewi_select_run_blocked"):
            def counted(*a):
                self.blocked += 1
                return fn(*a)
            return counted
        return fn


@gpu
def test_python_layer_equals_the_one_pick_form():
    import torch
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    for cls, kw in ((ExactIndex, {}), (DewiIndex, {"use_ann": False}), (IVFIndex, {"nlist": 16, "nprobe": 2})):
        idx, x, names, label, dewi, cols = ths.planted(cls, **kw)
        n = len(names)
        allow = np.arange(n) % 3 != 0
        seeds = [names[1], names[3], names[4]]
        for kwargs in ({}, {"max_sim": 0.95}, {"mmr_lambda": 0.3, "filter": allow, "seeds": seeds},
                       {"mmr_lambda": 1.0}, {"max_sim": 0.9, "filter": allow, "seeds": seeds}):
            want = idx.select_subset(60, return_gain=True, return_coverage=True, **kwargs)
            got = idx.select_subset_blocked(60, return_gain=True, return_coverage=True, picks_per_pass=32, **kwargs)
            assert got[0] == want[0] and got[2] == want[2], (cls.__name__, kwargs)
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
            assert idx.select_subset_blocked(60, picks_per_pass=4, **kwargs) == want[0]
            assert idx.select_subset_blocked(60, picks_per_pass=None, **kwargs) == want[0]
    # the device level: no blocked call for None / 1, fewer passes than picks, a bf16 corpus
    idx, x, names, label, dewi, cols = ths.planted(ExactIndex)
    c = idx._corpus
    real = c._lib
    c._lib = CountingLib(real)
    try:
        base = c.select_subset_device(50, 0.5, 0.95, seeds=[1, 3], return_coverage=True)
        one = c.select_subset_device(50, 0.5, 0.95, seeds=[1, 3], return_coverage=True, picks_per_pass=1)
        assert c._lib.blocked == 0
        out = c.select_subset_device(50, 0.5, 0.95, seeds=[1, 3], return_coverage=True, picks_per_pass=32, return_stats=True)
        assert c._lib.blocked >= 2
    finally:
        c._lib = real
    import wsguard
    wsguard.assert_bit_equal(one, base, "picks_per_pass = 1")
    wsguard.assert_bit_equal(out[:5], base, "picks_per_pass = 32")
    kk = int(base[2].item())
    stats = out[5]
    assert stats["picks_per_pass"] == 32 and 0 < stats["passes"] < kk and stats["rounds"] == stats["passes"], stats
    assert c.select_subset_device(50, 0.5, 0.95, return_stats=True)[-1] == {"rounds": 50, "passes": 50, "picks_per_pass": 1}
    from dewi._engine import DeviceCorpus
    E, rel = gaussian(True, True)
    cb = DeviceCorpus(E[:600].contiguous(), torch.from_numpy(rel[:600].copy()).cuda(), torch.zeros(600, device="cuda"), space="cosine")
    want = cb.select_subset_device(100, 0.5, 0.9, return_coverage=True)
    got = cb.select_subset_device(100, 0.5, 0.9, return_coverage=True, picks_per_pass=16, return_stats=True)
    wsguard.assert_bit_equal(got[:5], want, "bf16 corpus")
    assert got[5]["passes"] < int(want[2].item())
    with pytest.raises(ValueError, match="picks_per_pass"):
        cb.select_subset_device(10, picks_per_pass=0)


@gpu
def test_blocked_selection_after_remove_and_upsert_equals_a_fresh_index():
    from dewi.backends import ExactIndex
    _, x, names, label, dewi, cols = ths.planted(ExactIndex)
    n = len(names)
    idx = ExactIndex(dim=ths.DIM)
    idx.add_batch_columns(names, x, cols)
    idx.build()
    gone = [names[i] for i in range(0, n, 7)]
    idx.remove(gone)
    rs = np.random.RandomState(9)
    changed = [names[i] for i in range(1, n, 11) if names[i] not in gone]
    new_rows = rs.randn(len(changed) + 3, ths.DIM).astype(np.float32)
    new_ids = changed + ["new_a", "new_b", "new_c"]
    at = [names.index(d) for d in changed]
    new_cols = {k: np.concatenate([np.asarray(v)[at], np.asarray(v)[:3]]) for k, v in cols.items()}
    new_cols["dewi"] = 3.0 * rs.rand(len(new_ids))
    idx.upsert_batch_columns(new_ids, new_rows, new_cols)
    order = list(idx._doc_ids)
    src_x = {d: x[i] for i, d in enumerate(names)}
    src_c = {d: {k: np.asarray(v)[i] for k, v in cols.items()} for i, d in enumerate(names)}
    for j, d in enumerate(new_ids):
        src_x[d] = new_rows[j]
        src_c[d] = {k: v[j] for k, v in new_cols.items()}
    fresh = ExactIndex(dim=ths.DIM)
    fresh.add_batch_columns(order, np.stack([src_x[d] for d in order]), {k: np.array([src_c[d][k] for d in order]) for k in cols})
    fresh.build()
    for lam, max_sim in [(0.5, 0.95), (0.3, None), (1.0, None)]:
        got = idx.select_subset_blocked(40, lam, max_sim, return_gain=True)
        want = fresh.select_subset_blocked(40, lam, max_sim, return_gain=True)
        plain = fresh.select_subset(40, lam, max_sim, return_gain=True)
        assert got[0] == want[0] == plain[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[1], plain[1])


# ------------------------------------------------------------------------------------------------------------ 9. argument errors
@gpu
def test_argument_errors_come_before_any_device_work():
    import torch
    import wsguard
    _, E, _, rel = corpus("f32_64")
    n = 300
    E, rel = E[:n], rel[:n]
    nat, lib, dim, elem = lib_and_shape(E)
    bmax = int(lib.dewi_select_block_max(dim, elem))
    assert bmax >= 32 and int(lib.dewi_select_block_max(768, 0)) >= 32 and int(lib.dewi_select_block_max(768, 1)) >= 32
    assert int(lib.dewi_select_block_max(0, 0)) == 0 and int(lib.dewi_select_block_max(64, 2)) == 0
    need = int(lib.dewi_select_blocked_workspace_bytes(n, dim, elem, 8))
    assert need > 0 and int(lib.dewi_select_blocked_workspace_bytes(n, dim, elem, 0)) == 0
    assert int(lib.dewi_select_blocked_workspace_bytes(n, dim, elem, bmax + 1)) == 0
    ws = wsguard.GuardedBuffer(need, E.device, "0xff", "workspace")
    outs = [wsguard.GuardedOutput(s, t, E.device) for s, t in (((20,), torch.int64), ((20,), torch.float32), ((1,), torch.int64),
                                                               ((3,), torch.int64))]
    o_rows, o_gain, o_cnt, o_stats = outs
    rel_d = torch.from_numpy(np.ascontiguousarray(rel)).cuda()
    seeds_d = torch.tensor([1, 2, 3], dtype=torch.int64, device="cuda")
    stream = nat.stream_ptr()
    wsp = nat.ptr(ws.view)
    INVALID, WORKSPACE = -1, -3          # DEWI_ERR_INVALID_ARG, DEWI_ERR_WORKSPACE

    def run(block=8, ws_bytes=need, rows=nat.ptr(o_rows.mid), gain=nat.ptr(o_gain.mid), cnt=nat.ptr(o_cnt.mid), max_sim=0.9, lam=0.5,
            e=nat.ptr(E), r=nat.ptr(rel_d), n_rounds=4):
        return lib.dewi_select_run_blocked(e, elem, n, dim, r, 20, lam, max_sim, 0, rows, gain, cnt, None, None, wsp, ws_bytes, stream,
                                           block, n_rounds, nat.ptr(o_stats.mid))

    def seed(block=8, ws_bytes=need, max_sim=0.9, e=nat.ptr(E), s=nat.ptr(seeds_d)):
        return lib.dewi_select_seed_blocked(e, elem, n, dim, s, 3, max_sim, wsp, ws_bytes, stream, block)

    for rc, want in [(run(block=0), INVALID), (run(block=bmax + 1), INVALID), (run(ws_bytes=need - 1), WORKSPACE),
                     (run(rows=None), INVALID), (run(gain=None), INVALID), (run(cnt=None), INVALID), (run(e=None), INVALID),
                     (run(r=None), INVALID), (run(max_sim=float("nan")), INVALID), (run(lam=1.5), INVALID), (run(n_rounds=-1), INVALID),
                     (seed(block=0), INVALID), (seed(block=bmax + 1), INVALID), (seed(ws_bytes=need - 1), WORKSPACE),
                     (seed(max_sim=float("nan")), INVALID), (seed(e=None), INVALID), (seed(s=None), INVALID)]:
        assert rc == want, (rc, want)
    torch.cuda.synchronize()
    ws.check(interior=False)
    assert torch.equal(ws.view, torch.full_like(ws.view, 0xFF)), "an argument error touched the workspace"
    for o in outs:
        assert bool((o.full.view(torch.uint8) == wsguard.SENTINEL).all()), "an argument error touched an output"

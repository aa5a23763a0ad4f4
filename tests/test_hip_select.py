"""Subset selection on the GPU: ``dewi_select_begin`` / ``_seed`` / ``_run`` against tests/select_model.py.

A. Bit for bit at the ABI level on rows whose inner products are exact in any summation order (the recipe of
   test_hip_diverse.py::synthetic_rows: +-0.25 entries, every 8th row a copy of its predecessor, one all-NaN row), so that the
   model's float64 Gram matrix, rounded, is the device's fp32 g.  Rows, gains, the count, pen and owner are compared as bits
   (NaN == NaN, +-0 equal in pen), the prefill from ``kk`` on included.
B. The workspace contract: results do not depend on what the workspace held before, nothing outside it or the outputs is
   written.
C. Against the float64 model on gaussian corpora, up to the first pick that model does not decide by a margin.
D. Through ``ExactIndex`` / ``DewiIndex`` / ``IVFIndex`` on a corpus with planted clusters of copies.
"""
import itertools

import numpy as np
import pytest

import select_model as sm
import wsguard

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN_ROW = 5
N_MAX = 2053
NS = [1, 7, 300, 2053]          # fewer rows than waves (1, 7), a ragged last step, several steps per wave with a ragged tail
                                # (the grid shrinks with the corpus: at least four steps per wave where there are that many)
BUDGETS = [1, 5, 64, None]      # None: N + 3
LAMS = [0.0, 0.3, 0.5, 1.0]
MAX_SIMS = [INF, 0.9, 0.25]
# (name, bf16, dim, rows, element offset of the view inside its buffer)
CORPORA = [("f32_64", False, 64, N_MAX, 3 * 64), ("f32_50", False, 50, N_MAX, 3 * 50), ("f32_768", False, 768, N_MAX, 3 * 768),
           ("f32_1000", False, 1000, N_MAX, 3 * 1000), ("f32_8200", False, 8200, 96, 3 * 8200), ("bf16_64", True, 64, N_MAX, 3 * 64),
           ("bf16_100", True, 100, N_MAX, 3 * 100),
           ("f32_64_off1", False, 64, 300, 1)]        # whole units, but the view starts one element into a 16-byte unit
REL_VALUES = np.array([0.75, 0.5, 0.5, 0.25, 0.0, -0.0, -0.5, 0.625, 0.375, 0.375, INF, -INF, np.nan], np.float32)
_cache = {}


def synthetic_rows(n, dim, seed):
    """[n, dim] fp32: 16 nonzeros of +-0.25 per row — 12 in the first 20 columns (so that rows overlap: dots from -0.75 to
    0.75 in steps of 1/16), 4 in the rest, the LAST column among them for every other row (the tail of a row that is not whole
    16-byte units) —, every 8th row an exact copy of its predecessor, one all-NaN row."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, dim), np.float32)
    for i in range(n):
        head = rs.choice(20, 12, replace=False)
        tail = 20 + rs.choice(dim - 20, 4, replace=False)
        if i % 2:
            tail[0] = dim - 1
            while len(set(tail.tolist())) < 4:
                tail[1:] = 20 + rs.choice(dim - 21, 3, replace=False)
        rows[i, np.concatenate([head, tail])] = rs.choice(np.array([0.25, -0.25], np.float32), 16)
    rows[1::8] = rows[0::8][: rows[1::8].shape[0]]
    if n > NAN_ROW:
        rows[NAN_ROW] = np.nan
    return rows


def corpus(name):
    """(host rows fp32 [n, dim], device tensor [n, dim]: a view that starts at an odd row of — or one element into — a larger
    buffer, the fp32 Gram matrix, rel fp32 [n] with ties (a copy ties with its original), +-0, +-inf and NaN)"""
    import torch
    if name not in _cache:
        _, bf16, dim, n, off = next(c for c in CORPORA if c[0] == name)
        rows = synthetic_rows(n, dim, seed=dim)
        flat = torch.zeros(off + n * dim + 8, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        view = flat[off: off + n * dim].view(n, dim)
        view.copy_(torch.from_numpy(rows).cuda())          # (+-0.25, 0 and NaN are exact in bf16)
        with np.errstate(invalid="ignore"):
            gram = (rows.astype(np.float64) @ rows.astype(np.float64).T).astype(np.float32)
        rs = np.random.RandomState(dim + 1)
        rel = rs.choice(REL_VALUES, n)
        rel[1::8] = rel[0::8][: rel[1::8].shape[0]]
        _cache[name] = (rows, view, gram, rel, flat)
    return _cache[name][:4]


def device_select(E, n, rel, budgets, lam, max_sim, mask=None, seeds=None, id_offset=0, pattern="0xff", coverage=True):
    """begin, seeds, one run per entry of ``budgets`` on the same state.  Everything the library writes is guarded.  Returns
    (rows, gain — both of sum(budgets) positions, sentinel bytes where nothing was written —, kk, pen, owner)."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    dim, elem = int(E.shape[1]), 1 if E.dtype == torch.bfloat16 else 0
    total = max(int(sum(max(b, 0) for b in budgets)), 1)
    need = int(lib.dewi_select_workspace_bytes(n, dim, elem))
    assert need > 0
    ws = wsguard.GuardedBuffer(need, E.device, pattern, "select workspace")
    o_rows = wsguard.GuardedOutput((total,), torch.int64, E.device, label="rows")
    o_gain = wsguard.GuardedOutput((total,), torch.float32, E.device, label="gain")
    o_cnt = wsguard.GuardedOutput((1,), torch.int64, E.device, label="n_picked")
    o_pen = wsguard.GuardedOutput((n,), torch.float32, E.device, label="pen")
    o_own = wsguard.GuardedOutput((n,), torch.int64, E.device, label="owner")
    rel_d = torch.from_numpy(np.ascontiguousarray(rel)).cuda()
    mask_d = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda()
    stream = nat.stream_ptr()
    nat.check(lib.dewi_select_begin(n, dim, elem, nat.ptr(mask_d) if mask_d is not None else None, nat.ptr(ws.view), need, stream))
    if seeds is not None:
        seeds_d = torch.from_numpy(np.asarray(seeds, np.int64)).cuda()
        nat.check(lib.dewi_select_seed(nat.ptr(E), elem, n, dim, nat.ptr(seeds_d), len(seeds), max_sim, nat.ptr(ws.view), need, stream))
    for b in budgets:
        nat.check(lib.dewi_select_run(nat.ptr(E), elem, n, dim, nat.ptr(rel_d), b, lam, max_sim, id_offset, nat.ptr(o_rows.mid),
                                      nat.ptr(o_gain.mid), nat.ptr(o_cnt.mid), nat.ptr(o_pen.mid) if coverage else None,
                                      nat.ptr(o_own.mid) if coverage else None, nat.ptr(ws.view), need, stream))
    torch.cuda.synchronize()
    ws.check()
    for o in (o_rows, o_gain, o_cnt, o_pen, o_own):
        o.check_guards()
    if any(b > 0 for b in budgets):
        o_cnt.check_written()
        if coverage:
            o_pen.check_written()
            o_own.check_written()
    return (o_rows.mid.cpu().numpy(), o_gain.mid.cpu().numpy(), int(o_cnt.mid.cpu().numpy()[0]), o_pen.mid.cpu().numpy(),
            o_own.mid.cpu().numpy())


SENT_I64 = np.frombuffer(bytes([wsguard.SENTINEL] * 8), np.int64)[0]
SENT_U32 = np.frombuffer(bytes([wsguard.SENTINEL] * 4), np.uint32)[0]


def model_select(gram, n, rel, budgets, lam, max_sim, mask=None, seeds=None, id_offset=0):
    col = lambda s: gram[:n, s]          # noqa: E731
    st = sm.SelectState(n, mask)
    if seeds is not None:
        sm.seed(st, col, seeds, max_sim)
    rows, gains = [], []
    for b in budgets:
        r, g, _ = sm.run(st, col, rel, b, lam, max_sim, id_offset)
        rows.append(r)
        gains.append(g)
    return np.concatenate(rows), np.concatenate(gains).astype(np.float32), st


def assert_equal_to_model(got, want, id_offset=0, what=""):
    rows, gain, kk, pen, owner = got
    w_rows, w_gain, st = want
    assert kk == len(w_rows) == st.n_picked, (what, kk, len(w_rows))
    assert np.array_equal(rows[:kk], w_rows), (what, rows[:kk][:10], w_rows[:10])
    assert np.array_equal(gain[:kk].view(np.uint32), w_gain.view(np.uint32)), (what, gain[:kk][:10], w_gain[:10])
    assert (rows[kk:] == SENT_I64).all() and (gain[kk:].view(np.uint32) == SENT_U32).all(), f"{what}: the tail from {kk} on was written"
    assert np.array_equal((pen + np.float32(0)).view(np.uint32), (st.pen + np.float32(0)).view(np.uint32)), what
    assert np.array_equal(owner, np.where(st.owner >= 0, st.owner + id_offset, -1)), what


# ---------------------------------------------------------------------------------------------------------------- part A
CASES_A = [(c[0], n) for c in CORPORA if c[0] != "f32_64_off1" for n in (NS if c[3] == N_MAX else [c[3]])] + [("f32_64_off1", 300)]


@pytest.mark.parametrize("name,n", CASES_A, ids=[f"{c}-{n}" for c, n in CASES_A])
def test_bit_equal_to_the_model(name, n):
    _, E, gram, rel = corpus(name)
    E, rel = E[:n], rel[:n]
    short = 0
    for budget, lam, max_sim in itertools.product(BUDGETS, LAMS, MAX_SIMS):
        b = n + 3 if budget is None else budget
        got = device_select(E, n, rel, [b], lam, max_sim)
        want = model_select(gram, n, rel, [b], lam, max_sim)
        assert_equal_to_model(got, want, what=f"{name} n {n} budget {b} lambda {lam} max_sim {max_sim}")
        short += got[2] < min(b, n)
        if max_sim == 0.9:      # a copy ties with its original in rel and in every g: the lower row goes first, the copy is struck out
            picked = set(got[0][: got[2]].tolist())
            assert not any(r % 8 == 1 and r - 1 in picked for r in picked)
    if n >= 300:
        assert short > 0        # max_sim = 0.25 strikes nearly everything out: kk < budget was exercised


@pytest.mark.parametrize("name", ["f32_64", "f32_50", "f32_768", "bf16_100", "f32_8200"])
def test_masks_and_seeds(name):
    _, E, gram, rel = corpus(name)
    n = min(300, E.shape[0])
    E, rel = E[:n], rel[:n]
    rs = np.random.RandomState(3)
    half = rs.rand(n) < 0.5
    one = np.zeros(n, bool)
    one[11] = True
    masks = [half, np.zeros(n, bool), one, np.ones(n, bool)]
    excluded = int(np.flatnonzero(~half)[0])
    seed_lists = [None, [3], [excluded], [NAN_ROW], [8, 9, 200, excluded, n + 5, -1, 8]]    # (a copy pair, junk rows, a seed twice)
    for mask, seeds, (lam, max_sim) in itertools.product(masks, seed_lists, [(0.5, INF), (0.0, 0.9), (1.0, 0.25), (0.3, 0.9)]):
        got = device_select(E, n, rel, [20], lam, max_sim, mask=mask, seeds=seeds)
        want = model_select(gram, n, rel, [20], lam, max_sim, mask=mask, seeds=seeds)
        assert_equal_to_model(got, want, what=f"{name} mask {int(mask.sum())} seeds {seeds} lambda {lam} max_sim {max_sim}")
        assert mask[got[0][: got[2]]].all()
        if seeds:
            assert not set(got[0][: got[2]].tolist()) & set(seeds)


@pytest.mark.parametrize("name", ["f32_64", "f32_768", "bf16_64", "f32_50"])
def test_resume_and_id_offset(name):
    _, E, gram, rel = corpus(name)
    n = 300
    E, rel = E[:n], rel[:n]
    for (b1, b2), lam, max_sim in itertools.product([(1, 4), (7, 30), (30, 300), (5, 0)], [0.3, 1.0], [INF, 0.9]):
        whole = device_select(E, n, rel, [b1 + b2], lam, max_sim, seeds=[2], id_offset=1000)
        parts = device_select(E, n, rel, [b1, b2], lam, max_sim, seeds=[2], id_offset=1000)
        wsguard.assert_bit_equal(parts, whole, f"{name}: run({b1}) + run({b2}) against run({b1 + b2})")
        want = model_select(gram, n, rel, [b1, b2], lam, max_sim, seeds=[2], id_offset=1000)
        assert_equal_to_model(parts, want, id_offset=1000, what=f"{name} resume {b1}+{b2}")


def test_the_two_consequences():
    """lambda = 1 without a cut is the stable top-B of rel; lambda = 0 after one seed is farthest-first traversal."""
    rows, E, gram, rel = corpus("f32_64")
    n = 300
    got = device_select(E[:n], n, rel[:n], [40], 1.0, INF)
    order = [i for i in np.argsort(-sm.ord_f32(rel[:n]).astype(np.int64), kind="stable") if not np.isnan(rel[i])]
    assert got[0][: got[2]].tolist() == order[:40]
    ok = np.arange(n) != NAN_ROW
    got = device_select(E[:n], n, np.ones(n, np.float32), [12], 0.0, INF, seeds=[0], mask=ok)
    chosen, far = [0], []
    for _ in range(12):
        d = np.where(ok, gram[:n, chosen].max(axis=1), np.inf)
        d[chosen] = np.inf
        far.append(int(np.argmin(d)))                      # the row least similar to its nearest chosen row, lowest row first
        chosen.append(far[-1])
    assert got[0][:12].tolist() == far


# ---------------------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("name,n", [("f32_768", 300), ("f32_50", 2053), ("bf16_100", 300), ("f32_8200", 96)])
def test_workspace_contract(name, n):
    _, E, gram, rel = corpus(name)
    E, rel = E[:n], rel[:n]
    mask = np.arange(n) % 5 != 0
    for lam, max_sim in [(0.5, INF), (0.3, 0.9)]:
        base = None
        for pattern in wsguard.PATTERNS:
            got = device_select(E, n, rel, [10, 15], lam, max_sim, mask=mask, seeds=[4], pattern=pattern)   # (guards: device_select)
            if base is None:
                base = got
                assert_equal_to_model(got, model_select(gram, n, rel, [10, 15], lam, max_sim, mask=mask, seeds=[4]), what=name)
            wsguard.assert_bit_equal(got, base, f"{name}: workspace prefilled with {pattern}")


def test_cached_workspace_of_the_corpus_is_guarded():
    import torch
    from dewi._engine import DeviceCorpus
    rows, E, gram, rel = corpus("f32_768")
    n = 300
    c = DeviceCorpus(E[:n].contiguous(), torch.from_numpy(rel[:n].copy()).cuda(), torch.zeros(n, device="cuda"), space="cosine")
    first = c.select_subset_device(16, 0.5, 0.9, return_coverage=True)
    assert wsguard.guard(c) == 1
    for pattern in wsguard.PATTERNS:
        wsguard.poison(c, pattern)
        got = c.select_subset_device(16, 0.5, 0.9, return_coverage=True)
        torch.cuda.synchronize()
        wsguard.check(c)
        wsguard.assert_bit_equal(got, first, f"cached workspace prefilled with {pattern}")
    wsguard.release(c)
    want = model_select(gram, n, rel[:n], [16], 0.5, 0.9)
    kk = int(first[2].item())
    assert kk == len(want[0]) and first[0][:kk].cpu().numpy().tolist() == want[0].tolist()
    assert (first[0][kk:] == -1).all() and torch.isnan(first[1][kk:]).all()


# ---------------------------------------------------------------------------------------------------------------- part C
MARGIN = 2e-6      # the project's diverse-search margin
# The corpus seed of every case, chosen on the CPU (scripts/select_seeds.py: the lowest seed from 1 on) so that the float64 model
# ALONE decides at least three quarters of the picks before its first undecided one.
SHAPES_C = [(3000, 64, 48), (3000, 200, 48), (5000, 768, 32)]
SEEDS_C = {(3000, 200, False, 0.9, INF): 2, (3000, 200, False, 0.9, 0.8): 2, (3000, 200, True, 0.9, INF): 2,
           (3000, 200, True, 0.9, 0.8): 2}       # (n, dim, clustered, lambda, max_sim) -> seed; every other case: seed 1
CASES_C = [(n, d, b, cl, lam, ms) for (n, d, b) in SHAPES_C for cl in (False, True) for lam in (0.3, 0.5, 0.9) for ms in (INF, 0.8)]


def gaussian_corpus(n, dim, clustered, seed):
    """Unit rows fp32 and a dewi-like relevance in [0, 1): plain gaussian directions, or 200 gaussian centres (more than any budget here) with noise that
    puts the cosine inside a cluster near 0.9."""
    rs = np.random.RandomState(1000 * seed + dim)
    if clustered:
        centres = rs.randn(200, dim)
        centres /= np.linalg.norm(centres, axis=1, keepdims=True)
        x = centres[rs.randint(0, 200, n)] + (1.0 / 3.0) * rs.randn(n, dim) / np.sqrt(dim)
    else:
        x = rs.randn(n, dim)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return x, rs.rand(n).astype(np.float32)


def float64_model(n, dim, budget, clustered, lam, max_sim, seed):
    x, rel = gaussian_corpus(n, dim, clustered, seed)
    rows, gains, st, und = sm.select(x, rel, budget, lam, max_sim, dtype=np.float64)
    return x, rel, rows, gains, len(rows) if und is None else und


@pytest.mark.parametrize("n,dim,budget,clustered,lam,max_sim", CASES_C,
                         ids=[f"{n}x{d}-{'clustered' if cl else 'plain'}-lam{lam}-cut{ms}" for n, d, b, cl, lam, ms in CASES_C])
def test_against_the_float64_model(n, dim, budget, clustered, lam, max_sim):
    import torch
    seed = SEEDS_C.get((n, dim, clustered, lam, max_sim), 1)
    x, rel, w_rows, w_gains, decided = float64_model(n, dim, budget, clustered, lam, max_sim, seed)
    print(f"seed {seed}: the float64 model made {len(w_rows)} picks and decided {decided} before its first undecided one")
    assert len(w_rows) == budget and 4 * decided >= 3 * budget      # the floor holds on the model alone: no case passes empty
    big = torch.zeros((n + 1, dim), dtype=torch.float32, device="cuda")
    big[1:] = torch.from_numpy(x).cuda()
    rows, gain, kk, _, _ = device_select(big[1:], n, rel, [budget], lam, max_sim, coverage=False)
    assert kk == budget
    assert rows[:decided].tolist() == w_rows[:decided].tolist()
    err = np.abs(gain[:decided].astype(np.float64) - w_gains[:decided])
    print(f"largest gain error over the decided picks: {err.max():.3g}")
    assert err.max() <= 1e-5


def test_lambda_zero_with_one_seed_against_the_float64_model():
    """Without a seed step 0 is an exact all-zero tie that the tie rule, not a margin, decides: one seed row first."""
    import torch
    n, dim, budget = 3000, 64, 48
    x, rel = gaussian_corpus(n, dim, False, 1)
    w_rows, w_gains, _, und = sm.select(x, rel, budget, 0.0, INF, seeds=[17], dtype=np.float64)
    decided = budget if und is None else und
    assert 4 * decided >= 3 * budget
    rows, gain, kk, _, _ = device_select(torch.from_numpy(x).cuda(), n, rel, [budget], 0.0, INF, seeds=[17], coverage=False)
    assert kk == budget and rows[:decided].tolist() == w_rows[:decided].tolist()
    assert np.abs(gain[:decided].astype(np.float64) - w_gains[:decided]).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- part D
DIM, CLUSTERS, COPIES, SINGLES = 96, 24, 5, 30


def planted(cls, **kwargs):
    """An index of ``CLUSTERS`` x ``COPIES`` near-copies (noise 1e-3: similarity > 0.999) with differing dewi and ``SINGLES``
    single documents whose dewi lies below every cluster's best."""
    import dewi_oracle as orc
    key = ("planted", cls.__name__, tuple(sorted(kwargs.items())))
    if key not in _cache:
        rs = np.random.RandomState(41)
        centres = rs.randn(CLUSTERS, DIM).astype(np.float32)
        x = np.concatenate([np.repeat(centres, COPIES, axis=0) + 1e-3 * rs.randn(CLUSTERS * COPIES, DIM).astype(np.float32),
                            rs.randn(SINGLES, DIM).astype(np.float32)])
        label = np.concatenate([np.repeat(np.arange(CLUSTERS), COPIES), CLUSTERS + np.arange(SINGLES)])
        # clusters 0 .. 5 hold the 30 largest dewi values of the corpus: the plain top-B by dewi stays inside them
        dewi = np.concatenate([np.where(np.repeat(np.arange(CLUSTERS), COPIES) < 6, 1.3, 1.0) + 0.2 * rs.rand(CLUSTERS * COPIES),
                               0.2 * rs.rand(SINGLES)])
        perm = rs.permutation(x.shape[0])
        x, label, dewi = x[perm], label[perm], dewi[perm]
        n = x.shape[0]
        names = [f"doc_{i:04d}" for i in range(n)]
        cols = dict(orc.synth_payload_columns(n, seed=2), dewi=dewi.astype(np.float64))
        idx = cls(dim=DIM, **kwargs)
        idx.add_batch_columns(names, x, cols)
        idx.build()
        _cache[key] = (idx, x, names, label, dewi, cols)
    return _cache[key]


def cluster_coverage(selected_labels, all_labels):
    """reference metrics.cluster_coverage restated: the share of the clusters that have at least one selected member."""
    return len(set(selected_labels)) / len(set(all_labels))


def check_planted(idx):
    _, x, names, label, dewi, _ = idx
    idx = idx[0]
    lab = dict(zip(names, label.tolist()))
    dw = dict(zip(names, np.float32(dewi).tolist()))
    n = len(names)
    ids = idx.select_subset(n, mmr_lambda=0.5, max_sim=0.95)
    labs = [lab[d] for d in ids]
    assert len(set(labs)) == len(labs) == CLUSTERS + SINGLES                  # at most one per cluster, and every cluster
    for d in ids:                                                             # ... and it is the member with the highest dewi
        assert dw[d] == max(dw[m] for m in names if lab[m] == lab[d])
    clusters = label[label < CLUSTERS]
    ids = idx.select_subset(CLUSTERS, mmr_lambda=0.5)
    assert cluster_coverage([lab[d] for d in ids if lab[d] < CLUSTERS], clusters) == 1.0
    top = idx.select_subset(CLUSTERS, mmr_lambda=1.0)
    assert top == [names[i] for i in np.argsort(-np.float32(dewi), kind="stable")[:CLUSTERS]]
    assert cluster_coverage([lab[d] for d in top if lab[d] < CLUSTERS], clusters) < 1.0
    return ids


def test_planted_clusters_on_exact_index():
    import torch
    from dewi.backends import ExactIndex
    idx, x, names, label, dewi, cols = planted(ExactIndex)
    check_planted(planted(ExactIndex))
    corpus_ = idx._corpus
    n = len(names)
    # filter=, seeds=, relevance=, return_gain and return_coverage against the device-level call
    allow = np.arange(n) % 3 != 0
    rel = np.random.RandomState(5).rand(n).astype(np.float32)
    seeds = [names[1], names[3]]
    ids, gain, near, sim = idx.select_subset(20, 0.4, 0.9, relevance=rel, filter=allow, seeds=seeds, return_gain=True,
                                             return_coverage=True)
    r, g, kk, pen, owner = corpus_.select_subset_device(20, 0.4, 0.9, torch.from_numpy(rel).cuda(), torch.from_numpy(allow).cuda(),
                                                        [1, 3], return_coverage=True)
    kk = int(kk.item())
    assert ids == [names[i] for i in r[:kk].tolist()] and np.array_equal(gain, g[:kk].cpu().numpy())
    assert near == [names[o] if o >= 0 else None for o in owner.tolist()]
    assert np.array_equal(sim.view(np.uint32), pen.cpu().numpy().view(np.uint32))
    assert all(allow[names.index(d)] for d in ids) and not set(ids) & set(seeds)
    stored = idx._corpus.emb.cpu().numpy()
    want = sm.select(stored, rel, 20, 0.4, 0.9, mask=allow, seeds=[1, 3], dtype=np.float64)
    und = len(want[0]) if want[3] is None else want[3]
    assert und > 0 and ids[:und] == [names[i] for i in want[0][:und]]
    # the other spellings of the filter, the relevance as a tensor, the allow-list of the subset
    for f in (idx.make_filter(allow), [names[i] for i in np.flatnonzero(allow)], np.flatnonzero(allow)):
        assert idx.select_subset(20, 0.4, 0.9, relevance=torch.from_numpy(rel).cuda(), filter=f, seeds=seeds) == ids
    assert len(idx.make_filter(doc_ids=ids)) == len(ids)
    assert idx.select_subset(n + 10, 1.0) == [names[i] for i in np.argsort(-np.float32(dewi), kind="stable")]
    assert idx.select_subset(0) == []
    with pytest.raises(ValueError, match="mmr_lambda"):
        idx.select_subset(5, mmr_lambda=1.5)
    with pytest.raises(KeyError):
        idx.select_subset(5, seeds=["no such doc"])


def test_planted_clusters_through_the_facade_and_the_ivf_index():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    want = check_planted(planted(ExactIndex))
    assert check_planted(planted(DewiIndex, use_ann=False)) == want
    assert check_planted(planted(IVFIndex, nlist=16, nprobe=2)) == want
    assert IVFIndex.select_subset is ExactIndex.select_subset


def test_l2_raises():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.types import Payload
    q = np.ones(4, np.float32)
    for idx in (ExactIndex(dim=4, space="l2"), DewiIndex(dim=4, space="l2")):
        idx.add("a", q, Payload())
        with pytest.raises(NotImplementedError, match="l2"):
            idx.select_subset(1)


def test_selection_after_remove_and_upsert_equals_a_fresh_index():
    from dewi.backends import ExactIndex
    _, x, names, label, dewi, cols = planted(ExactIndex)
    n = len(names)
    idx = ExactIndex(dim=DIM)
    idx.add_batch_columns(names, x, cols)
    idx.build()
    gone = [names[i] for i in range(0, n, 7)]
    idx.remove(gone)
    rs = np.random.RandomState(9)
    changed = [names[i] for i in range(1, n, 11) if names[i] not in gone]
    new_rows = rs.randn(len(changed) + 3, DIM).astype(np.float32)
    new_ids = changed + ["new_a", "new_b", "new_c"]
    at = [names.index(d) for d in changed]
    new_cols = {k: np.concatenate([np.asarray(v)[at], np.asarray(v)[:3]]) for k, v in cols.items()}
    new_cols["dewi"] = 3.0 * rs.rand(len(new_ids))
    idx.upsert_batch_columns(new_ids, new_rows, new_cols)
    # the same documents, built afresh in the mutated index's row order
    order = list(idx._doc_ids)
    src_x = {d: x[i] for i, d in enumerate(names)}
    src_c = {d: {k: np.asarray(v)[i] for k, v in cols.items()} for i, d in enumerate(names)}
    for j, d in enumerate(new_ids):
        src_x[d] = new_rows[j]
        src_c[d] = {k: v[j] for k, v in new_cols.items()}
    fresh = ExactIndex(dim=DIM)
    fresh.add_batch_columns(order, np.stack([src_x[d] for d in order]),
                            {k: np.array([src_c[d][k] for d in order]) for k in cols})
    fresh.build()
    for lam, max_sim in [(0.5, 0.95), (0.3, None), (1.0, None)]:
        got = idx.select_subset(40, lam, max_sim, return_gain=True)
        want = fresh.select_subset(40, lam, max_sim, return_gain=True)
        assert got[0] == want[0] and np.array_equal(got[1], want[1])

"""GPU tests of the two-launch robust fit (csrc/robust_fit_fast.hip) that know WHICH code produced a result.

The fit falls back to an exact whole-column select whenever its bracket missed or a buffer overflowed, so a test that
compares only medians cannot see a wrong tail branch behind a column that fell back, nor tell that a branch is never
reached.  Here every call goes through the raw ABI (``dewi_robust_fit_f32``) on a guarded, poisoned workspace, and after it
the column's counters (``dewi_robust_fit_fast_plan`` says where they are) are held to the NumPy model of
tests/fit_fast_model.py: ``ticket``, ``fallback``, ``lt eqlo eqhi nan``, ``bucket[16]`` and ``overflow``, next to the
median and the MAD bit for bit against NumPy.  tests/test_fit_fast_model_host.py proves on the CPU that the cases between
them take every route of the tail, both overflows and the missed bracket.
"""
import functools
import warnings

import numpy as np
import pytest

import fit_fast_model as fm
import wsguard

pytestmark = pytest.mark.gpu
WORDS = 32                                 # uint32 words of one counter record
LT, EQLO, EQHI, NAN, OVERFLOW, TICKET, FALLBACK, PAD, BUCKET = 0, 1, 2, 3, 4, 5, 6, 7, 8


def numpy_fit(x):
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        med = np.median(x)
        return np.float32(med), np.float32(np.median(np.abs(x - med)))


def device_table(host, mis):
    """The (n_signals, ld) fp32 table on the device with its first element ``mis`` floats past a 16-byte boundary."""
    import torch
    flat = torch.full((host.size + 8,), 1e9, dtype=torch.float32, device="cuda")
    shift = (mis - (flat.data_ptr() & 15) // 4) % 4
    view = flat[shift: shift + host.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(host).reshape(-1)))
    assert (view.data_ptr() & 15) // 4 == mis
    return view


def fit_twice(host, n, mis=0, pattern="0xff"):
    """``dewi_robust_fit_f32`` twice over the columns ``host[s, :n]`` on ONE guarded workspace (the second call meets what the
    first left); yields (call, medians, MADs, counters [2][n_signals][32]) after each call, guards checked."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    ns, ld = host.shape
    plan = nat.fit_fast_plan(n, ns)
    assert plan["supported"] == 1 and plan["counters_bytes"] == 4 * WORDS
    dev = device_table(host, mis)
    need = int(lib.dewi_robust_fit_workspace_bytes(ns))
    ws = wsguard.GuardedBuffer(need, "cuda", pattern, label="fit workspace")
    med = wsguard.GuardedOutput((ns,), torch.float32, "cuda", label="medians")
    mad = wsguard.GuardedOutput((ns,), torch.float32, "cuda", label="MADs")
    off, size = plan["counters_offset"], 2 * ns * plan["counters_bytes"]
    for call in range(2):
        for o in (med, mad):
            o.full.view(torch.uint8).fill_(wsguard.SENTINEL)
        nat.check(lib.dewi_robust_fit_f32(nat.ptr(dev), n, ld, ns, nat.ptr(med.mid), nat.ptr(mad.mid), nat.ptr(ws.view), need,
                                          nat.stream_ptr()))
        torch.cuda.synchronize()
        ws.check()
        med.check()
        mad.check()
        ctr = ws.view[off: off + size].cpu().numpy().view(np.uint32).reshape(2, ns, WORDS).astype(np.int64)
        yield call, med.mid.cpu().numpy(), mad.mid.cpu().numpy(), ctr


def check_column(x, plan, mis, got_med, got_mad, ctr, what):
    """One column of one call against NumPy and the model; returns the two phases' models."""
    want_med, want_mad = numpy_fit(x)
    m0 = fm.model(x, None, plan, mis)
    assert fm.same_f32(got_med, want_med), (what, got_med, want_med, fm.describe(m0))
    m1 = fm.model(x, got_med, plan, mis)                     # the device's own median: NumPy's, as just shown
    assert fm.same_f32(got_mad, want_mad), (what, got_mad, want_mad, fm.describe(m1))
    for phase, m in (("median", m0), ("MAD", m1)):
        c = ctr[0 if phase == "median" else 1]
        tag = (what, phase, fm.describe(m))
        print(f"{what} {phase}: {fm.describe(m)}; device fallback {c[FALLBACK]} overflow {c[OVERFLOW]} ticket {c[TICKET]}")
        assert c[TICKET] == plan["slices"], tag
        assert c[FALLBACK] == m["fallback"], tag
        assert (c[LT], c[EQLO], c[EQHI], c[NAN]) == (m["lt"], m["eqlo"], m["eqhi"], m["nan"]), tag
        assert c[BUCKET: BUCKET + plan["buckets"]].tolist() == m["bucket"].tolist(), tag
        if m["overflow"] is None:                            # past a bucket's capacity: the count depends on the order
            assert c[OVERFLOW] > 0, tag
        else:
            assert c[OVERFLOW] == m["overflow"], tag
    return m0, m1


@pytest.mark.parametrize("i", range(len(fm.CASES)), ids=[c.id for c in fm.CASES])
def test_single_column_takes_its_route(i):
    from dewi import _native as nat
    case = fm.CASES[i]
    plan = nat.fit_fast_plan(case.n, 1)
    x = case.column(plan)
    for call, med, mad, ctr in fit_twice(x[None, :], case.n, case.mis, wsguard.PATTERNS[i % len(wsguard.PATTERNS)]):
        m0, _ = check_column(x, plan, case.mis, med[0], mad[0], ctr[:, 0], f"{case.id} call {call}")
        if isinstance(case.pin, tuple):
            assert (m0["k0_route"], m0["k1_route"]) == case.pin
        else:
            assert m0["causes"] == (case.pin,)


@pytest.mark.parametrize("pad", [1, 3])
def test_four_routes_stacked_with_a_leading_dimension(pad):
    """ties_low_half, ties_high_half, two_clusters and straddle_adjacent as the columns of one table whose leading dimension
    puts them at all four misalignments; the padding behind a column must not be read."""
    from dewi import _native as nat
    n, ns = 65_538, 4
    ld = n + pad
    plan = nat.fit_fast_plan(n, ns)
    assert plan["slices"] == 16
    cols = [fm.ties_low_half(n, 1), fm.ties_high_half(n, 1), fm.two_clusters(n, 1), fm.straddle_adjacent(n, plan, 1)]
    pins = [("eqlo", "next-bucket-from-eqlo"), ("bucket-regs", "eqhi"), ("bucket-regs", "next-bucket-skipping-empty"),
            ("bucket-regs", "next-bucket-from-bucket")]
    host = np.full((ns, ld), 1e9, np.float32)
    for s, x in enumerate(cols):
        host[s, :n] = x
    assert sorted((s * ld) % 4 for s in range(ns)) == [0, 1, 2, 3]
    for call, med, mad, ctr in fit_twice(host, n, 0, "random"):
        for s, x in enumerate(cols):
            m0, _ = check_column(x, plan, (s * ld) % 4, med[s], mad[s], ctr[:, s], f"column {s} ld n+{pad} call {call}")
            assert (m0["k0_route"], m0["k1_route"]) == pins[s], (s, fm.describe(m0))


def test_a_column_that_overflows_leaves_its_neighbour_on_the_bracket_path():
    """2 x 1.1M: the one-bin column next to a gamma column.  With two signals a column has 128 workgroups, whose staging
    (512 keys a bucket) cannot fill a bucket's 65 536 keys: the one-bin column overflows the staging here (the capacity
    overflow exists at one signal only: CASES).  Its neighbour must stay on the bracket path and exact, the guards intact."""
    from dewi import _native as nat
    n, ns = 1_100_000, 2
    plan = nat.fit_fast_plan(n, ns)
    cols = [fm.one_bin(n), fm.gamma(n)]
    host = np.stack(cols)
    for call, med, mad, ctr in fit_twice(host, n, 0, "0x7f"):
        m0, _ = check_column(cols[0], plan, 0, med[0], mad[0], ctr[:, 0], f"one_bin call {call}")
        assert m0["causes"] == ("lds-overflow",)
        g0, g1 = check_column(cols[1], plan, (n % 4), med[1], mad[1], ctr[:, 1], f"gamma call {call}")
        assert g0["bracket_ok"] and g1["bracket_ok"]


def test_the_threshold_between_one_workgroup_and_the_bracket():
    """n = 65 536: one workgroup per column selects, nobody takes a ticket or touches a counter; one value more: the bracket."""
    from dewi import _native as nat
    x = fm.gauss(65_537, 9)
    small = x[:65_536]
    plan = nat.fit_fast_plan(len(small), 1)
    assert plan["slices"] == 1 and len(small) == plan["small_n"]
    for call, med, mad, ctr in fit_twice(small[None, :], len(small), 0, "0xff"):
        want_med, want_mad = numpy_fit(small)
        assert fm.same_f32(med[0], want_med) and fm.same_f32(mad[0], want_mad)
        assert not ctr.any(), ctr                            # zeroed by the launcher, then left alone
    plan = nat.fit_fast_plan(len(x), 1)
    for call, med, mad, ctr in fit_twice(x[None, :], len(x), 0, "0xff"):
        m0, m1 = check_column(x, plan, 0, med[0], mad[0], ctr[:, 0], f"65537 call {call}")
        assert ctr[0, 0, TICKET] == ctr[1, 0, TICKET] == plan["slices"] == 16 and m0["bracket_ok"] and m1["bracket_ok"]


# ---- what the counters say about the existing suite's columns: fallback == model, nothing else ---------------------------
@functools.lru_cache(maxsize=None)
def table_fallbacks(kind, n):
    """(names, columns, plan, device medians, device fallback flags [2][n_signals]) of one table fitted once."""
    from dewi import _native as nat
    if kind == "adversarial":
        cols = fm.adversarial_columns(n)
    else:
        import dewi_oracle as orc
        c64 = orc.synth_payload_columns(n, seed=5)
        cols = {k: c64[k].astype(np.float32) for k in orc.SIGNAL_KEYS}
    names = list(cols)
    host = np.stack([cols[k] for k in names])
    plan = nat.fit_fast_plan(n, len(names))
    call, med, mad, ctr = next(iter(fit_twice(host, n, 0, "zeros")))
    return names, host, plan, med, ctr[:, :, FALLBACK].copy()


def check_fallback(kind, n, s):
    names, host, plan, med, fallback = table_fallbacks(kind, n)
    x, mis = host[s], (s * n) % 4
    want_med, _ = numpy_fit(x)
    assert fm.same_f32(med[s], want_med)
    for phase, m in enumerate((fm.model(x, None, plan, mis), fm.model(x, med[s], plan, mis))):
        print(f"FALLBACK-TABLE | {kind} | {n} | {names[s]} | {'MAD' if phase else 'median'} | "
              f"{'fallback' if fallback[phase, s] else 'bracket'} | {', '.join(m['causes']) or '-'} | model: {fm.describe(m)}")
        assert fallback[phase, s] == m["fallback"], (names[s], phase, fm.describe(m))


@pytest.mark.parametrize("s", range(12))
@pytest.mark.parametrize("n", [100_003, 400_000])
def test_adversarial_columns_fall_back_where_the_model_says(n, s):
    """The twelve columns of test_hip_scorer.py::test_fast_fit_adversarial_columns_stay_exact, laid out as that test lays
    them out (one table, ld = n).  As measured on an MI355X, device and model agreeing on all 48 (column, phase) pairs:

    n = 100 003 (8 of 24 fall back): sorted_up, sorted_down, slow_drift in both phases by staging overflow;
    outliers_on_the_sampled_runs in both by a missed bracket; the other eight columns stay on the bracket path, every one
    with k1 = same-rank (n is odd).
    n = 400 000 (13 of 24): the same four; blocks in both phases, periodic_outliers, bimodal and mixed_nan in the median
    phase, all by staging overflow.  Of the eleven on the bracket path, six have both middles '== lo' (heavy_zero,
    few_values, constant), one both '== hi' (mixed_nan's MAD), and four select in a bucket held in registers.
    No pair overflows a bucket's capacity or takes a next-bucket route; one selects in a bucket read from memory."""
    check_fallback("adversarial", n, s)


@pytest.mark.parametrize("s", range(7))
def test_c5_columns_fall_back_where_the_model_says(s):
    """The seven synthetic signal columns of configuration C5 at 1M rows (test_score_1m_rows_matches_oracle).  As measured:
    none of the 14 (column, phase) pairs falls back; all select inside one bucket (11 from memory, 3 in registers)."""
    check_fallback("c5", 1_000_000, s)

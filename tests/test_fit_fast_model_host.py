"""The NumPy model of the two-launch robust fit (tests/fit_fast_model.py) on the CPU: its finished values against
``np.median`` bit for bit, its counters against naive Python loops, and the COVERAGE CONDITION of the GPU tests
(tests/test_hip_fit_fast_paths.py): every case takes the route it is named for, and together the cases take every route of
the kernel's tail, both overflows and the missed bracket.  Without that condition the GPU tests could pass through the
whole-column fallback alone.  The plan comes from the library (``dewi_robust_fit_fast_plan``: host only, no GPU)."""
import ctypes
import functools
import struct
import warnings

import numpy as np
import pytest

import fit_fast_model as fm


def plan_of(n, n_signals=1):
    from dewi import _native as nat
    return nat.fit_fast_plan(n, n_signals)


def numpy_fit(x):
    """(median, MAD) as scorer.py computes them: NumPy in the column's own fp32."""
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        med = np.median(x)
        return np.float32(med), np.float32(np.median(np.abs(x - med)))


@functools.lru_cache(maxsize=None)
def phases_of(i):
    """(column, plan, median model, MAD model) of CASES[i]."""
    case = fm.CASES[i]
    plan = plan_of(case.n)
    x = case.column(plan)
    m0 = fm.model(x, None, plan, case.mis)
    return x, plan, m0, fm.model(x, m0["value"], plan, case.mis)


# ---- the accessor ------------------------------------------------------------------------------------------------------
def test_plan_words():
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    p = plan_of(1_000_000, 7)
    assert p["supported"] == 1 and p["slices"] == 36 and p["counters_bytes"] == 128
    assert (p["small_n"], p["sample"], p["delta"], p["buckets"]) == (65536, 4096, 208, 16)
    assert p["bucket_cap"] * p["buckets"] == 1 << 20 and p["reg_keys"] == 8192 and p["bucket_lds"] == 512
    for n, ns, slices in ((65_536, 1, 1), (65_537, 1, 16), (65_538, 4, 16), (1_100_000, 1, 256), (1_100_000, 2, 128),
                          (400_000, 12, 21), (100_003, 12, 21), (70_000, 300, 1)):
        assert plan_of(n, ns)["slices"] == slices, (n, ns)
    assert plan_of(6_000_000, 1)["supported"] == 0 and plan_of(1, 1024)["supported"] == 1 and plan_of(1, 1025)["supported"] == 0
    for ns in (1, 2, 7, 12):
        p = plan_of(100_000, ns)
        need = int(lib.dewi_robust_fit_workspace_bytes(ns))
        compact = 4 * ns * p["bucket_cap"] * p["buckets"]                  # the buckets follow the counters (256-byte steps)
        assert p["counters_offset"] % 256 == 0
        assert p["counters_offset"] + 2 * ns * p["counters_bytes"] + compact <= need
    # a shorter buffer gets the first words only
    out = (ctypes.c_int64 * 4)(-7, -7, -7, -7)
    assert lib.dewi_robust_fit_fast_plan(1_000_000, 7, out, 2) == 0
    assert list(out) == [1, 36, -7, -7]


# ---- the result --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(fm.CASES)), ids=[c.id for c in fm.CASES])
def test_case_values_are_numpys_and_the_median_phase_takes_its_route(i):
    case = fm.CASES[i]
    x, plan, m0, m1 = phases_of(i)
    med, mad = numpy_fit(x)
    print(f"{case.id}: median {fm.describe(m0)}; MAD {fm.describe(m1)}")
    assert fm.same_f32(m0["value"], med), (m0["value"], med)
    assert fm.same_f32(m1["value"], mad), (m1["value"], mad)
    if isinstance(case.pin, tuple):
        assert m0["bracket_ok"] and (m0["k0_route"], m0["k1_route"]) == case.pin, fm.describe(m0)
    else:
        assert m0["causes"] == (case.pin,), fm.describe(m0)


def test_named_routes_hold_what_the_issue_says_of_them():
    """Details of single cases that a label does not carry."""
    by_id = {c.id: i for i, c in enumerate(fm.CASES)}
    _, plan, m0, _ = phases_of(by_id["two_clusters-n65538-mis0"])
    assert m0["bshift"] == 28 and 1 < m0["k1_bucket"] < plan["buckets"] - 1
    for name in ("far_clusters-n65538-mis0", "far_clusters-n69632-mis3"):           # the walk stops at its bound
        _, plan, m0, _ = phases_of(by_id[name])
        assert m0["k1_bucket"] == plan["buckets"] - 1 and not m0["bucket"][1:-1].any() and m0["bucket"][0] > 0
    x, plan, m0, _ = phases_of(by_id["one_bin-n65538-mis0"])
    assert (m0["span"], m0["bshift"], m0["lt"]) == (0x3FF, 6, 0) and m0["eqlo"] + m0["eqhi"] + m0["bucket"].sum() == len(x)
    x, plan, m0, _ = phases_of(by_id["ties_low_half-n65538-mis0"])
    assert m0["lo"] == fm.ord_f32(np.float32([0.5]))[0] and m0["eqlo"] == len(x) // 2
    x, plan, m0, _ = phases_of(by_id["ties_high_half-n65538-mis0"])
    assert m0["hi"] == fm.ord_f32(np.float32([fm.W_HI]))[0] and m0["eqhi"] == len(x) // 2
    x, plan, m0, m1 = phases_of(by_id["one_bin-n1100000-mis0"])
    assert not m0["lds_over"].any() and m0["cap_over"].all() and m0["overflow"] is None      # every bucket, by capacity alone
    x, plan, m0, m1 = phases_of(by_id["runs_outliers-n65538-mis0"])
    assert not m0["lds_over"].any() and not m0["cap_over"].any() and m0["overflow"] == 0
    for name in ("nan_unsampled-n65537-mis0", "nan_sampled-n65538-mis0"):
        x, plan, m0, m1 = phases_of(by_id[name])
        assert m0["nan"] == 1 and m0["fallback"] == 0 and np.isnan(m0["value"]) and np.isnan(m1["value"])
    x, plan, m0, m1 = phases_of(by_id["inf_majority-n65538-mis0"])
    assert m0["value"] == np.inf and np.isnan(m1["value"])
    # at two signals a column of 1.1M rows has 128 workgroups of at most 512 keys a bucket: 65 536 keys, the capacity itself.
    # The capacity overflow exists at one signal only; next to a second column the same data overflows the staging.
    p2 = plan_of(1_100_000, 2)
    assert p2["slices"] * p2["bucket_lds"] <= p2["bucket_cap"]
    assert fm.model(fm.one_bin(1_100_000), None, p2)["causes"] == ("lds-overflow",)
    g = fm.model(fm.gamma(1_100_000), None, p2, mis=0)
    assert g["bracket_ok"]


def test_coverage_condition():
    """Every route label, both overflow causes and the missed bracket are reached by a named case."""
    k0, k1, causes = {}, {}, {}
    for i, case in enumerate(fm.CASES):
        for phase, m in zip(("median", "MAD"), phases_of(i)[2:]):
            where = f"{case.id} {phase}"
            if m["fallback"]:
                for c in m["causes"]:
                    causes.setdefault(c, where)
            else:
                k0.setdefault(m["k0_route"], where)
                k1.setdefault(m["k1_route"], where)
    for what, want, got in (("k0 route", fm.K0_LABELS, k0), ("k1 route", fm.K1_LABELS, k1), ("fallback cause", fm.CAUSES, causes)):
        for label in want:
            assert label in got, f"no case reaches the {what} {label!r}"
            print(f"{what} {label}: {got[label]}")
        assert set(got) <= set(want), set(got) - set(want)


# ---- small columns under a small plan: every route and cause within a few hundred values ----------------------------------
SMALL = dict(supported=1, slices=3, small_n=0, sample=64, delta=5, buckets=16, bucket_lds=8, bucket_cap=20, reg_keys=12)


def small_column(rs):
    """50 .. 400 values with forced ties; the spread of the keys varies from one 22-bit bin to many."""
    n = int(rs.randint(50, 400))
    kind = rs.randint(0, 5)
    if kind == 0:
        x = 1 + rs.randint(0, 1024, n) * 2.0 ** -23                       # one bin
    elif kind == 1:
        x = rs.randint(-3, 4, n) * 0.25                                   # a handful of values around zero
    elif kind == 2:
        x = np.round(rs.randn(n), 1)
    elif kind == 3:
        x = np.concatenate([np.full((n + 1) // 2, 0.5), 0.5 + rs.randint(1, 50, n // 2) * 2.0 ** -14])   # the lower half ties
        rs.shuffle(x)
    else:
        x = rs.gamma(2, 0.5, n)
        x[rs.randint(0, n, n // 4)] = x[0]
    x = x.astype(np.float32)
    if rs.rand() < 0.1:
        x[rs.randint(0, n)] = rs.choice([np.nan, np.inf, -np.inf])
    return x


def test_small_random_columns_with_ties_equal_numpy():
    rs = np.random.RandomState(11)
    seen = set()
    for _ in range(400):
        x = small_column(rs)
        plan = dict(SMALL, slices=int(rs.randint(1, 6)))
        mis = int(rs.randint(0, 4))
        med, mad = numpy_fit(x)
        m0 = fm.model(x, None, plan, mis)
        m1 = fm.model(x, m0["value"], plan, mis)
        assert fm.same_f32(m0["value"], med) and fm.same_f32(m1["value"], mad), (x.tolist(), plan, mis)
        for m in (m0, m1):
            seen.update(m["causes"] if m["fallback"] else (("k0", m["k0_route"]), ("k1", m["k1_route"])))
    want = set(fm.CAUSES) | {("k0", r) for r in fm.K0_LABELS} | {("k1", r) for r in fm.K1_LABELS}
    assert seen == want, want - seen              # the small plan reaches all of the model's branches, too


def naive_key(v):
    """The key of one fp32 value from its bits."""
    if v != v:
        return 0xFFFFFFFF
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    if u == 0x80000000:
        u = 0                                      # -0 -> +0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def test_counters_equal_naive_loops():
    rs = np.random.RandomState(12)
    for _ in range(60):
        x = small_column(rs)
        n = len(x)
        plan = dict(SMALL, slices=int(rs.randint(1, 6)))
        mis = int(rs.randint(0, 4))
        med = None if rs.rand() < 0.5 else numpy_fit(x)[0]
        m = fm.model(x, med, plan, mis)
        vals = [float(v) for v in x] if med is None else [float(abs(np.float32(v) - np.float32(med))) for v in x]
        keys = [naive_key(v) for v in vals]
        assert keys == m["keys"].tolist()
        # the sample: run r of 16 starts at the multiple of 16 at or below the middle of the r-th of 4 parts
        pos = []
        for r in range(plan["sample"] // 16):
            start = ((2 * r + 1) * n // (2 * (plan["sample"] // 16))) // 16 * 16
            pos += [min(start + j, n - 1) for j in range(16)]
        assert pos == m["pos"].tolist()
        sample = sorted(keys[p] for p in pos)
        lo = sample[plan["sample"] // 2 - plan["delta"]] & ~0x3FF
        hi = sample[plan["sample"] // 2 + plan["delta"]] | 0x3FF
        assert (lo, hi) == (m["lo"], m["hi"])
        # every element through the slice that takes it: head, 16-byte units, tail
        head = min((4 - mis) % 4, n)
        n4 = (n - head) // 4
        owner = [None] * n
        for i in range(head):
            owner[i] = 0
        for s in range(plan["slices"]):
            for unit in range(n4 * s // plan["slices"], n4 * (s + 1) // plan["slices"]):
                for j in range(4):
                    assert owner[head + 4 * unit + j] is None
                    owner[head + 4 * unit + j] = s
        for i in range(head + 4 * n4, n):
            owner[i] = plan["slices"] - 1
        lt = eqlo = eqhi = nan = 0
        per_slice = [[0] * 16 for _ in range(plan["slices"])]
        for i, (v, k) in enumerate(zip(vals, keys)):
            nan += v != v
            if k < lo:
                lt += 1
            elif k == lo:
                eqlo += 1
            elif k == hi:
                eqhi += 1
            elif k < hi:
                per_slice[owner[i]][(k - lo - 1) >> m["bshift"]] += 1
        assert (lt, eqlo, eqhi, nan) == (m["lt"], m["eqlo"], m["eqhi"], m["nan"])
        assert per_slice == m["per_slice"].tolist()
        bucket = [sum(row[b] for row in per_slice if row[b] <= plan["bucket_lds"]) for b in range(16)]
        assert bucket == m["bucket"].tolist()
        over = sum(row[b] > plan["bucket_lds"] for row in per_slice for b in range(16))
        if any(c > plan["bucket_cap"] for c in bucket):
            assert m["overflow"] is None and "capacity-overflow" in m["causes"]
        else:
            assert m["overflow"] == over and ("lds-overflow" in m["causes"]) == (over > 0)
        # the span's top four bits: the last key inside lands in a bucket below 16, and bshift is the smallest such shift
        assert (hi - 1 - lo - 1) >> m["bshift"] < 16 and (m["bshift"] == 0 or (hi - lo - 2) >> (m["bshift"] - 1) >= 8)

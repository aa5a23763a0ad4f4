"""A NumPy model of ONE phase of the two-launch robust fit (csrc/robust_fit_fast.hip), word for word what the kernel does
with a column: the keys, the sampled positions, the bracket [lo, hi], the counters of the one pass, the staging of every
workgroup, the check of the bracket, and the ROUTE by which the last workgroup of the column picks the two middle keys.

The fit is exact whatever happens, because a column whose bracket missed or whose buffers overflowed is selected over as a
whole instead.  That fallback hides a wrong tail branch from a test that compares only medians: this model says which code
produced the number, so that the GPU tests (tests/test_hip_fit_fast_paths.py) can hold ``Counters.fallback`` and the
counters themselves to it.  Plain NumPy, int64 keys, no cleverness: the kernel's code is the specification of the bracket,
``np.median`` the specification of the result (tests/test_fit_fast_model_host.py holds the model to the latter).

``plan`` is the dict of ``dewi._native.fit_fast_plan(n, n_signals)`` (``dewi_robust_fit_fast_plan``): nothing here repeats
a constant of the kernel.  ``mis`` is the column's misalignment in floats: ``(address & 15) // 4``.

The module also holds the column builders of the two test files: each is named for the route it pins.
"""
import numpy as np

K0_LABELS = ("eqlo", "eqhi", "bucket-regs", "bucket-memory")
K1_LABELS = ("same-rank", "eqlo", "eqhi", "same-bucket-equal", "same-bucket-min-above-regs", "same-bucket-min-above-memory",
             "next-bucket-from-eqlo", "next-bucket-from-bucket", "next-bucket-skipping-empty")
CAUSES = ("lds-overflow", "capacity-overflow", "missed")
RUN = 16                                   # the sample is runs of 16 consecutive values (one 64-byte line each)
PREFIX_DROP = 10                           # the bracket's ends are 22-bit key prefixes


# ---- keys --------------------------------------------------------------------------------------------------------------
def ord_f32(x):
    """Ascending integer keys of fp32 values as int64: -0 counts as +0, every NaN is 0xFFFFFFFF (common.hpp ord_f32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        u = (x + np.float32(0)).view(np.uint32).astype(np.int64)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    k[np.isnan(x)] = 0xFFFFFFFF
    return k


def unord_f32(k):
    """The fp32 value of a key (common.hpp unord_f32)."""
    k = int(k)
    u = (k & 0x7FFFFFFF) if (k & 0x80000000) else (~k & 0xFFFFFFFF)
    return np.array([u], np.uint32).view(np.float32)[0]


def phase_values(x, med):
    """What a phase orders: the column (``med`` None: the median phase) or the fp32 ``|x - med|`` (the MAD phase)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if med is None:
        return x
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.float32(med)).astype(np.float32)


def finish_value(k0, k1, n, nans):
    """fp32 result from the two middle keys: odd n the lower one, even n the fp32 mean; any NaN in the column -> NaN."""
    if nans:
        return np.float32(np.nan)
    a, b = unord_f32(k0), unord_f32(k1)
    if n & 1:
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(np.float32(a + b) * np.float32(0.5))


# ---- the bracket -------------------------------------------------------------------------------------------------------
def sample_positions(n, plan):
    """Positions of the sampled values, as the kernel forms them: run r of 16 around the middle of the r-th of sample / 16
    equal parts of the column, its start rounded down to a multiple of 16, every position clamped to n - 1."""
    i = np.arange(plan["sample"], dtype=np.int64)
    runs = plan["sample"] // RUN
    centre = ((2 * (i // RUN) + 1) * n) // (2 * runs)
    pos = (centre & ~np.int64(RUN - 1)) + (i % RUN)
    return np.minimum(pos, n - 1)


def bracket(keys, plan):
    """(lo, hi, span, bshift): the 22-bit prefixes of the sorted sample's ranks sample / 2 -/+ delta, lo's low bits clear and
    hi's set; a key strictly inside has bucket (key - lo - 1) >> bshift, the top log2(buckets) of the span's bits."""
    sk = np.sort(keys[sample_positions(len(keys), plan)])
    half, delta = plan["sample"] // 2, plan["delta"]
    lo = (int(sk[half - delta]) >> PREFIX_DROP) << PREFIX_DROP
    hi = ((int(sk[half + delta]) >> PREFIX_DROP) << PREFIX_DROP) | ((1 << PREFIX_DROP) - 1)
    span = hi - lo
    span_bits = (span - 1).bit_length() if span > 1 else 1
    bucket_bits = plan["buckets"].bit_length() - 1
    bshift = span_bits - bucket_bits if span_bits > bucket_bits else 0
    return lo, hi, span, bshift


def slice_bounds(n, mis, slices):
    """[(first, end)] of the elements each workgroup of a column takes: the head up to 16-byte alignment goes to slice 0,
    the body's 16-byte units are split ``n4 * s // slices``, the tail behind the last whole unit goes to the last slice."""
    head = min((4 - mis) % 4, n)
    n4 = (n - head) // 4
    out = []
    for s in range(slices):
        a, b = head + 4 * (n4 * s // slices), head + 4 * (n4 * (s + 1) // slices)
        out.append((0 if s == 0 else a, n if s == slices - 1 else b))
    return out


# ---- one phase ---------------------------------------------------------------------------------------------------------
def model(x, med, plan, mis=0):
    """One phase over the fp32 column ``x`` (``med`` None: median; else MAD around ``med``).  Returns a dict:

    ``keys pos lo hi span bshift``; the counters ``lt eqlo eqhi nan`` and ``inside[16]`` (every key strictly inside the
    bracket, per bucket); ``per_slice[slices][16]``, ``lds_over[slices][16]`` (workgroup s staged more than bucket_lds keys
    of bucket b and published none of them), ``bucket[16]`` (what the workgroups published: ``Counters.bucket``),
    ``cap_over[16]`` (the published keys exceed a bucket's capacity), ``overflow`` (``Counters.overflow``, or None where it
    depends on the order of the workgroups: after a capacity overflow); ``bracket_ok``, ``fallback``, ``causes``;
    ``k0_route k1_route`` (None after a fallback), ``k1_bucket`` (on the next-bucket routes), ``k0 k1 value``."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = len(x)
    assert n > plan["small_n"], "columns of up to small_n values take no bracket: one workgroup selects over them"
    B, slices = plan["buckets"], plan["slices"]
    v = phase_values(x, med)
    keys = ord_f32(v)
    nan = int(np.isnan(v).sum())
    lo, hi, span, bshift = bracket(keys, plan)
    out = dict(n=n, keys=keys, pos=sample_positions(n, plan), lo=lo, hi=hi, span=span, bshift=bshift, nan=nan)
    out["lt"] = lt = int((keys < lo).sum())
    out["eqlo"] = eqlo = int((keys == lo).sum())
    out["eqhi"] = eqhi = int((keys == hi).sum()) if hi != lo else 0       # lo == hi: such a key counts as "== lo"
    inside = (keys > lo) & (keys < hi)
    bk = np.where(inside, (keys - lo - 1) >> bshift, -1)
    assert bk.max() < B
    out["inside"] = np.bincount(bk[inside], minlength=B).astype(np.int64)
    per_slice = np.zeros((slices, B), np.int64)
    for s, (a, b) in enumerate(slice_bounds(n, mis, slices)):
        part = bk[a:b]
        per_slice[s] = np.bincount(part[part >= 0], minlength=B)
    assert np.array_equal(per_slice.sum(axis=0), out["inside"])           # every element exactly once
    lds_over = per_slice > plan["bucket_lds"]
    bc = np.where(lds_over, 0, per_slice).sum(axis=0)                     # a workgroup adds its count only if it fits
    cap_over = bc > plan["bucket_cap"]                                    # ... and the add that crosses the capacity sees it
    out.update(per_slice=per_slice, lds_over=lds_over, bucket=bc, cap_over=cap_over)
    out["overflow"] = None if cap_over.any() else int(lds_over.sum())
    r0, r1 = (n - 1) // 2, n // 2
    # ascending layout of the column: [below lo | == lo | bucket 0 .. 15 | == hi | above hi]
    a0 = lt
    a1 = a0 + eqlo
    a2 = a1 + int(bc.sum())
    a3 = a2 + eqhi
    overflowed = bool(lds_over.any() or cap_over.any())
    missed = not (r0 >= a0 and r1 < a3)
    out["bracket_ok"] = ok = not overflowed and not missed
    out["fallback"] = 0 if ok else 1
    out["causes"] = tuple(c for c, on in zip(CAUSES, (lds_over.any(), cap_over.any(), not overflowed and missed)) if on)
    out["k0_route"] = out["k1_route"] = None
    if not ok:                                                            # whole_column(): exact by one workgroup
        sk = np.sort(keys)
        k0, k1 = int(sk[r0]), int(sk[r1])
    else:
        reg_keys = plan["reg_keys"]

        def bucket_keys(b):
            return np.sort(keys[bk == b])

        b0k, rin0, below0, eq0, kb = -1, 0, 0, 0, None
        if r0 < a1:
            k0, out["k0_route"] = lo, "eqlo"
        elif r0 >= a2:
            k0, out["k0_route"] = hi, "eqhi"
        else:
            acc = a1
            for b in range(B):
                if r0 < acc + bc[b]:
                    b0k, rin0 = b, r0 - acc
                    break
                acc += bc[b]
            kb = bucket_keys(b0k)
            k0 = int(kb[rin0])
            below0 = int(np.searchsorted(kb, k0, side="left"))
            eq0 = int(np.searchsorted(kb, k0, side="right")) - below0
            out["k0_route"] = "bucket-regs" if bc[b0k] <= reg_keys else "bucket-memory"
        if r1 == r0:
            k1, out["k1_route"] = k0, "same-rank"
        elif r1 < a1:
            k1, out["k1_route"] = lo, "eqlo"
        elif r1 >= a2:
            k1, out["k1_route"] = hi, "eqhi"
        elif b0k >= 0 and rin0 + 1 < bc[b0k]:                             # the next rank is in the same bucket
            if rin0 + 1 < below0 + eq0:
                k1, out["k1_route"] = k0, "same-bucket-equal"
            else:
                k1 = int(kb[kb > k0].min())
                out["k1_route"] = "same-bucket-min-above-" + ("regs" if bc[b0k] <= reg_keys else "memory")
        else:                                                             # first key of the next non-empty bucket
            b = b0k + 1
            while b < B - 1 and bc[b] == 0:
                b += 1
            k1 = int(bucket_keys(b).min())
            out["k1_bucket"] = b
            out["k1_route"] = ("next-bucket-skipping-empty" if b > b0k + 1 else
                               "next-bucket-from-eqlo" if b0k < 0 else "next-bucket-from-bucket")
    out.update(k0=k0, k1=k1, value=finish_value(k0, k1, n, nan))
    return out


def describe(m):
    """One line on a phase: its path, and the route or the cause."""
    if m["fallback"]:
        return "fallback: " + ", ".join(m["causes"])
    return f"bracket: k0 {m['k0_route']}, k1 {m['k1_route']}"


def same_f32(a, b):
    """Bit-equal fp32 values; a NaN matches a NaN."""
    a, b = np.float32(a), np.float32(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32))


# ---- column builders ---------------------------------------------------------------------------------------------------
W_HI = np.array([0x3F8003FF], np.uint32).view(np.float32)[0]      # its key ends in 0x3FF: a bracket's upper key


def ties_low_half(n, seed=0):
    """Even n: n/2 copies of 0.5 (its key ends in ten zero bits, so lo IS that key), the rest 0.51 + gamma above them.
    The lower middle is '== lo', the upper middle the smallest key of the first bucket that holds any."""
    assert n % 2 == 0
    rs = np.random.RandomState(1000 + seed)
    x = np.concatenate([np.full(n // 2, 0.5, np.float32), (0.51 + rs.gamma(2, 0.5, n // 2)).astype(np.float32)])
    rs.shuffle(x)
    return x


def ties_high_half(n, seed=0):
    """Even n: n/2 copies of the float 0x3F8003FF (hi IS its key), the rest strictly below: the lower middle sits in a
    bucket, the upper middle is '== hi'."""
    assert n % 2 == 0
    rs = np.random.RandomState(2000 + seed)
    x = np.concatenate([np.full(n // 2, W_HI, np.float32), (W_HI - np.float32(0.01) - rs.gamma(2, 0.5, n // 2)).astype(np.float32)])
    rs.shuffle(x)
    return x


def two_clusters(n, seed=0):
    """Even n: exactly n/2 values in N(-50, 1) and n/2 in N(50, 1).  The middles are the largest key of the lower cluster
    and the smallest of the upper one, with empty buckets between them (the keys around 0 span 2^31: bshift 28)."""
    assert n % 2 == 0
    rs = np.random.RandomState(3000 + seed)
    x = np.concatenate([rs.randn(n // 2) - 50, rs.randn(n // 2) + 50]).astype(np.float32)
    rs.shuffle(x)
    return x


def far_clusters(n, seed=0):
    """Even n: n/2 values in [1, 1.01] and n/2 in [1.95, 1.99].  The bracket spans nearly the whole binade (2^23 keys,
    bshift 19): the lower middle ends bucket 0, the upper middle is the first key of bucket 15, the LAST one, behind
    fourteen empty buckets: the walk over empty buckets ends at its bound, not at a count."""
    assert n % 2 == 0
    rs = np.random.RandomState(3500 + seed)
    x = np.concatenate([rs.uniform(1, 1.01, n // 2), rs.uniform(1.95, 1.99, n // 2)]).astype(np.float32)
    rs.shuffle(x)
    return x


def straddle_adjacent(n, plan, seed=0):
    """Even n: uniform(1, 2), then UNSAMPLED positions only (the bracket cannot move) rewritten until exactly n/2 keys lie
    below the first key of the median's bucket: the lower middle is the last key of one bucket, the upper middle the first
    of the next."""
    assert n % 2 == 0
    rs = np.random.RandomState(4000 + seed)
    x = rs.uniform(1, 2, n).astype(np.float32)
    keys = ord_f32(x)
    lo, hi, span, bshift = bracket(keys, plan)
    b = (int(np.sort(keys)[n // 2]) - lo - 1) >> bshift
    assert 1 <= b < plan["buckets"], b
    edge = lo + 1 + (b << bshift)                                 # the first key of bucket b
    need = n // 2 - int((keys < edge).sum())
    assert 0 <= need < n // 8, need
    free = np.ones(n, bool)
    free[sample_positions(n, plan)] = False
    order = np.argsort(-keys, kind="stable")                      # the largest keys first: far above the bracket
    move = order[free[order]][:need]
    assert (keys[move] >= edge).all()
    below = edge - 5                                              # a key of bucket b - 1
    assert below > lo and (below - lo - 1) >> bshift == b - 1
    x[move] = unord_f32(below)
    assert int((ord_f32(x) < edge).sum()) == n // 2
    return x


def one_bin(n, seed=0):
    """1 + j * 2^-23 with j uniform in 0 .. 1023: the whole column inside one 22-bit bin, so lo and hi are its two ends
    (span 0x3FF, bshift 6) and the 16 buckets hold 64 distinct keys each: heavy ties."""
    rs = np.random.RandomState(5000 + seed)
    return (1 + rs.randint(0, 1024, n) * 2.0 ** -23).astype(np.float32)


def gauss(n, seed=0):
    return np.random.RandomState(6000 + seed).randn(n).astype(np.float32)


def gamma(n, seed=0):
    return np.random.RandomState(7000 + seed).gamma(2, 0.5, n).astype(np.float32)


def runs_outliers(n, plan, seed=0):
    """N(0, 1) with every SAMPLED value -1e6: the bracket sits on the outliers and misses both middles; nothing overflows."""
    x = gauss(n, 100 + seed)
    x[sample_positions(n, plan)] = -1e6
    return x


def nan_unsampled(n, plan, seed=0):
    """gamma with one NaN where the sample does not look."""
    x = gamma(n, 200 + seed)
    free = np.ones(n, bool)
    free[sample_positions(n, plan)] = False
    x[np.flatnonzero(free)[n // 3]] = np.nan
    return x


def nan_sampled(n, plan, seed=0):
    """gamma with one NaN at a sampled position."""
    x = gamma(n, 300 + seed)
    x[sample_positions(n, plan)[plan["sample"] // 3]] = np.nan
    return x


def inf_majority(n, seed=0):
    """60 % +inf: the median is inf, and |x - inf| is NaN wherever x is inf."""
    rs = np.random.RandomState(8000 + seed)
    return np.where(rs.rand(n) < 0.6, np.inf, rs.randn(n)).astype(np.float32)


def adversarial_columns(n):
    """The twelve columns of tests/test_hip_scorer.py::test_fast_fit_adversarial_columns_stay_exact, value for value (the
    same draws from the same RandomState(n) in the same order)."""
    rs = np.random.RandomState(n)
    stride = n // 8192
    periodic = rs.randn(n).astype(np.float32)
    periodic[(np.arange(8192) * 2 + 1) * n // (2 * 8192)] = 1e6
    runs = rs.randn(n).astype(np.float32)
    run_start = (((2 * np.arange(256) + 1) * n) >> 9) & ~15
    runs[np.minimum((run_start[:, None] + np.arange(16)[None, :]).ravel(), n - 1)] = -1e6
    heavy_zero = np.where(rs.rand(n) < 0.7, 0.0, rs.gamma(2, 0.5, n)).astype(np.float32)
    few_values = rs.choice(np.array([0.25, 0.5, 0.75], np.float32), n)
    bimodal = np.where(np.arange(n) % 2 == 0, rs.randn(n) - 50, rs.randn(n) + 50).astype(np.float32)
    return {
        "sorted_up": np.sort(rs.randn(n).astype(np.float32)),
        "sorted_down": np.sort(rs.randn(n).astype(np.float32))[::-1].copy(),
        "periodic_outliers": periodic,
        "outliers_on_the_sampled_runs": runs,
        "slow_drift": (np.linspace(-3, 3, n) + 0.01 * rs.randn(n)).astype(np.float32),
        "heavy_zero": heavy_zero,
        "few_values": few_values,
        "constant": np.full(n, 3.25, np.float32),
        "bimodal": bimodal,
        "blocks": np.repeat(rs.randn(n // stride + 1).astype(np.float32), stride)[:n].copy(),
        "negatives": (-rs.gamma(2, 0.5, n)).astype(np.float32),
        "mixed_nan": np.where(np.arange(n) == n // 3, np.nan, rs.randn(n)).astype(np.float32),
    }


# ---- the cases of the two test files -----------------------------------------------------------------------------------
class Case:
    """One column and what its MEDIAN phase must do: ``pin`` is ``(k0 route, k1 route)`` on the bracket path or the name
    of a fallback cause.  The MAD phase does whatever the model says; both phases count towards the coverage condition."""

    def __init__(self, name, n, build, pin, mis=0, needs_plan=False):
        self.name, self.n, self.build, self.pin, self.mis, self.needs_plan = name, n, build, pin, mis, needs_plan
        self.id = f"{name}-n{n}-mis{mis}"

    def column(self, plan):
        return self.build(self.n, plan) if self.needs_plan else self.build(self.n)


N_EVEN = (65_538, 69_632)              # the smallest even size on the two-launch path, and a multiple of every tile
CASES = [Case(name, n, build, pin, mis, needs_plan)
         for name, build, pin, needs_plan in (
             ("ties_low_half", ties_low_half, ("eqlo", "next-bucket-from-eqlo"), False),
             ("ties_high_half", ties_high_half, ("bucket-regs", "eqhi"), False),
             ("two_clusters", two_clusters, ("bucket-regs", "next-bucket-skipping-empty"), False),
             ("straddle_adjacent", straddle_adjacent, ("bucket-regs", "next-bucket-from-bucket"), True),
             ("one_bin", one_bin, ("bucket-regs", "same-bucket-equal"), False))
         for n in N_EVEN for mis in (0, 1, 3)]
CASES += [
    Case("far_clusters", 65_538, far_clusters, ("bucket-regs", "next-bucket-skipping-empty")),
    Case("far_clusters", 69_632, far_clusters, ("bucket-regs", "next-bucket-skipping-empty"), mis=3),
    Case("one_bin", 150_000, one_bin, ("bucket-memory", "same-bucket-equal")),             # a bucket of more than 8192 keys
    Case("gauss", 200_000, gauss, ("bucket-memory", "same-bucket-min-above-memory")),
    Case("gauss", 65_537, gauss, ("bucket-regs", "same-rank")),
    Case("gauss", 65_538, gauss, ("bucket-regs", "same-bucket-min-above-regs"), mis=2),
    Case("one_bin", 1_100_000, one_bin, "capacity-overflow"),      # 256 workgroups stage ~270 keys a bucket, 68 750 in all
    Case("runs_outliers", 65_538, runs_outliers, "missed", needs_plan=True),
    Case("runs_outliers", 100_003, runs_outliers, "missed", mis=1, needs_plan=True),
    Case("nan_unsampled", 65_537, nan_unsampled, ("bucket-regs", "same-rank"), needs_plan=True),
    Case("nan_sampled", 65_538, nan_sampled, ("bucket-regs", "same-bucket-min-above-regs"), needs_plan=True),
    Case("inf_majority", 65_538, inf_majority, ("eqlo", "eqlo")),
    Case("inf_majority", 65_537, inf_majority, ("eqlo", "same-rank"), mis=3),
]

"""Facets, the host side (no GPU): the NumPy model (``facet_model.py``) against plain Python loops and against the reference's
``stratify_by_dewi`` as recorded in ``tests/golden/facets_stratify.json``; the edge rules (closed last bin, -0 / +0, infinite
edges, NaN keys and values, the 64-bit key subtraction); ``Facet`` and ``resolve_bins``; the four symbols in header /
``EXPORTED_SYMBOLS`` / the library; the plan's path limits and the argument errors, which come before any device work.
"""
import ctypes
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

import facet_model as fm

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "facets_stratify.json"
NEW = {"dewi_facet_workspace_bytes", "dewi_facet_plan", "dewi_facet_tuning_set", "dewi_facet_run"}


# ------------------------------------------------------------------------------------------ the model against plain loops
def loop_slot(x, kind, n_bins, key_lo, edges):
    if kind == fm.KEY_I32_RANGE:
        b = int(x) - int(key_lo)
        return b if 0 <= b < n_bins else n_bins
    if kind == fm.KEY_F32_EDGES and math.isnan(float(x)):
        return n_bins + 1
    for i in range(n_bins):                                          # the reference's loop (metrics.py:152-161)
        lo, hi = edges[i], edges[i + 1]
        if (lo <= x <= hi) if i == n_bins - 1 else (lo <= x < hi):
            return i
    return n_bins


def loop_facet(keys, kind, n_bins, key_lo, edges, sels, values):
    s = n_bins + 2
    out = []
    for rows in sels:
        rec = [{"count": 0, "vals": []} for _ in range(s)]
        for r in rows:
            slot = loop_slot(keys[r], kind, n_bins, key_lo, edges)
            rec[slot]["count"] += 1
            if values is not None and not (values.dtype == np.float32 and math.isnan(float(values[r]))):
                rec[slot]["vals"].append(values[r])
        out.append(rec)
    return out


def signed_zero_key(v):
    """Total order of fp32 bits as a sortable Python key (-0 below +0)."""
    return (float(v), 0 if math.copysign(1.0, float(v)) < 0 else 1)


@pytest.mark.parametrize("kind", [fm.KEY_I32_RANGE, fm.KEY_I32_EDGES, fm.KEY_F32_EDGES])
@pytest.mark.parametrize("sel", [fm.SEL_ALL, fm.SEL_MASKS, fm.SEL_LISTS])
@pytest.mark.parametrize("vtype", [None, np.int32, np.float32])
def test_model_equals_plain_loops(kind, sel, vtype):
    rs = np.random.RandomState(100 * kind + 10 * sel + (0 if vtype is None else vtype().itemsize + (vtype == np.float32)))
    n, n_bins, p = 300, 7, 3
    key_lo, edges = -3, None
    if kind == fm.KEY_I32_RANGE:
        keys = rs.randint(-6, 8, n).astype(np.int32)
    elif kind == fm.KEY_I32_EDGES:
        edges = np.array([-5, -2, -1, 0, 3, 4, 6, 9], dtype=np.int32)
        keys = rs.randint(-8, 12, n).astype(np.int32)
    else:
        edges = np.array([-np.inf, -1.5, -0.0, 0.25, 0.5, 1.0, 2.0, 3.0], dtype=np.float32)
        keys = rs.choice(np.array([-np.inf, -2, -1.5, -0.0, 0.0, 0.25, 0.3, 1.0, 3.0, 3.5, np.inf, np.nan], dtype=np.float32), n)
    values = None
    if vtype is np.int32:
        values = rs.choice(np.array([fm.INT32_MIN, -7, 0, 5, fm.INT32_MAX], dtype=np.int32), n)
    elif vtype is np.float32:
        values = rs.choice(np.array([-np.inf, -1.0, -0.0, 0.0, 1e-3, 7.5, np.nan], dtype=np.float32), n)
    masks = rows = lims = None
    if sel == fm.SEL_ALL:
        sels = [list(range(n))]
    elif sel == fm.SEL_MASKS:
        masks = (rs.rand(p, n) < 0.4).astype(np.uint8) * rs.randint(1, 256, (p, n)).astype(np.uint8)
        masks[1] = 0
        sels = [[r for r in range(n) if masks[j, r]] for j in range(p)]
    else:
        segs = [rs.randint(-5, n + 5, 200).tolist(), [], rs.randint(0, 4, 50).tolist()]
        rows = np.array(sum(segs, []), dtype=np.int64)
        lims = np.cumsum([0] + [len(s) for s in segs])
        sels = [[r for r in s if 0 <= r < n] for s in segs]
    got = fm.facet(keys, kind, n_bins, key_lo, edges, sel, masks, rows, lims, values)
    want = loop_facet(keys, kind, n_bins, key_lo, edges, sels, values)
    assert got["counts"].shape == (len(sels), n_bins + 2)
    for j, rec in enumerate(want):
        assert got["counts"][j].tolist() == [r["count"] for r in rec]
        if values is None:
            continue
        for s, r in enumerate(rec):
            v = r["vals"]
            assert got["vcount"][j, s] == len(v)
            if not v:
                assert got["vmin"][j, s] == (np.inf if vtype is np.float32 else fm.INT32_MAX)
                assert got["vmax"][j, s] == (-np.inf if vtype is np.float32 else fm.INT32_MIN)
                continue
            lo, hi = min(v, key=signed_zero_key), max(v, key=signed_zero_key)
            assert got["vmin"][j, s].tobytes() == np.asarray(lo).tobytes() and got["vmax"][j, s].tobytes() == np.asarray(hi).tobytes()
            if vtype is np.int32:
                assert int(got["vsum"][j, s]) == sum(int(x) for x in v)
            else:
                with np.errstate(invalid="ignore"):
                    want_sum = math.fsum(float(x) for x in v) if all(math.isfinite(float(x)) for x in v) else float(np.sum(np.asarray(v, np.float64)))
                assert got["vsum"][j, s] == want_sum or (math.isnan(got["vsum"][j, s]) and math.isnan(want_sum))
    if kind != fm.KEY_F32_EDGES:
        assert not got["counts"][:, n_bins + 1].any()               # int keys have no NaN


# ------------------------------------------------------------------------------------------ the edge rules, one by one
def test_last_bin_is_closed_and_zeros_are_equal():
    e = np.array([-1.0, 0.0, 1.0], dtype=np.float32)
    keys = np.array([-1.0, -0.0, 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(-1.0), np.float32(-2.0))],
                    dtype=np.float32)
    assert fm.slots_of(keys, fm.KEY_F32_EDGES, 2, edges=e).tolist() == [0, 1, 1, 1, 2, 2]
    e = np.array([-0.0, 1.0], dtype=np.float32)                      # an edge of -0 takes +0, an edge of +0 takes -0
    assert fm.slots_of(np.array([0.0, -0.0], np.float32), fm.KEY_F32_EDGES, 1, edges=e).tolist() == [0, 0]
    ei = np.array([0, 10, 20], dtype=np.int32)
    assert fm.slots_of(np.array([-1, 0, 9, 10, 20, 21], np.int32), fm.KEY_I32_EDGES, 2, edges=ei).tolist() == [2, 0, 0, 1, 1, 2]


def test_infinite_edges_and_nan_keys():
    e = np.array([-np.inf, 0.0, np.inf], dtype=np.float32)
    keys = np.array([-np.inf, -1e38, 0.0, 1e38, np.inf, np.nan], dtype=np.float32)
    assert fm.slots_of(keys, fm.KEY_F32_EDGES, 2, edges=e).tolist() == [0, 0, 1, 1, 1, 3]
    c = fm.facet(keys, fm.KEY_F32_EDGES, 2, edges=e)["counts"][0]
    assert c.tolist() == [2, 3, 0, 1]


def test_key_subtraction_is_64_bit():
    keys = np.array([fm.INT32_MIN, -1, 0, fm.INT32_MAX], dtype=np.int32)
    assert fm.slots_of(keys, fm.KEY_I32_RANGE, 4, key_lo=fm.INT32_MAX).tolist() == [4, 4, 4, 0]      # no wrap to bin 1
    assert fm.slots_of(keys, fm.KEY_I32_RANGE, 4, key_lo=fm.INT32_MIN).tolist() == [0, 4, 4, 4]
    assert fm.slots_of(keys, fm.KEY_I32_RANGE, 2, key_lo=-1).tolist() == [2, 0, 1, 2]


def test_nan_values_are_left_out_and_negative_zero_sits_below_zero():
    keys = np.zeros(6, dtype=np.int32)
    vals = np.array([np.nan, 0.0, -0.0, np.nan, 2.0, -0.0], dtype=np.float32)
    got = fm.facet(keys, fm.KEY_I32_RANGE, 1, values=vals)
    assert got["counts"][0].tolist() == [6, 0, 0] and got["vcount"][0].tolist() == [4, 0, 0]
    assert np.signbit(got["vmin"][0, 0]) and got["vmin"][0, 0] == 0.0 and got["vmax"][0, 0] == 2.0
    assert got["vsum"][0, 0] == 2.0 and got["vmin"][0, 1] == np.inf and got["vmax"][0, 2] == -np.inf
    allnan = fm.facet(keys, fm.KEY_I32_RANGE, 1, values=np.full(6, np.nan, np.float32))
    assert allnan["vcount"].sum() == 0 and allnan["vmin"][0, 0] == np.inf and allnan["vmax"][0, 0] == -np.inf and allnan["vsum"][0, 0] == 0.0


def test_int_sum_is_exact_beyond_int32():
    keys = np.zeros(5, dtype=np.int32)
    vals = np.full(5, fm.INT32_MAX, dtype=np.int32)
    assert int(fm.facet(keys, fm.KEY_I32_RANGE, 1, values=vals)["vsum"][0, 0]) == 5 * fm.INT32_MAX


# ------------------------------------------------------------------------------------------ the reference, as recorded
def golden():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    return np.asarray(g["dewi_times_64"], dtype=np.float64) / 64.0, g["cases"]


def test_model_equals_the_reference_stratify_fixture():
    dewi, cases = golden()
    assert dewi.astype(np.float32).astype(np.float64).tolist() == dewi.tolist()      # exact in fp32
    assert {c["name"] for c in cases} >= {"all", "inner_bins", "two_rankings_with_repeats", "empty"}
    on_edge = 0
    for c in cases:
        rows = np.asarray(sum(c["segments"], []), dtype=np.int64)
        got = fm.stratify(dewi, c["bins"], rows)
        want = {(lo, hi): v for lo, hi, v in c["expected"]}
        assert got == want, c["name"]                                # the same integer count over the same total: equal floats
        on_edge += int(np.isin(dewi[rows], c["bins"]).sum())
    assert on_edge > 100


# ------------------------------------------------------------------------------------------ Facet and bins
def test_facet_top_orders_ties_by_key():
    from dewi.facets import Facet
    f = Facet("site", ["a", "b", "c", "d"], [3, 5, 3, 5], other=2, nan=1)
    assert f.total == 19
    assert f.top() == [("b", 5), ("d", 5), ("a", 3), ("c", 3)]
    assert f.top(1) == [("b", 5)] and f.top(0) == []
    assert f.proportions() == {"a": 3 / 19, "b": 5 / 19, "c": 3 / 19, "d": 5 / 19}
    assert f.as_dict()["counts"] == [3, 5, 3, 5] and f.as_dict()["total"] == 19 and "stats" not in f.as_dict()
    assert Facet("x", [1], [0], 0, 0).proportions() == {1: 0.0}


def test_bins_validation():
    from dewi import _native as nat
    from dewi.facets import resolve_bins
    b = resolve_bins("cat", ["a", "b", "c"], None)
    assert (b.key_kind, b.n_bins, b.key_lo, b.edges, b.keys) == (0, 3, 0, None, ["a", "b", "c"])
    b = resolve_bins("int", None, None, min_max=lambda: (1990, 2025))
    assert (b.n_bins, b.key_lo, b.keys[0], b.keys[-1]) == (36, 1990, 1990, 2025)
    b = resolve_bins("int", None, (-2, 2))
    assert (b.key_kind, b.n_bins, b.key_lo, b.keys) == (0, 5, -2, [-2, -1, 0, 1, 2])
    b = resolve_bins("int", None, [0, 10, 20])
    assert b.key_kind == 1 and b.edges.dtype == np.int32 and b.keys == [(0, 10), (10, 20)]
    b = resolve_bins("float", None, [0.0, 0.25, 1.0])
    assert b.key_kind == 2 and b.edges.dtype == np.float32 and b.keys == [(0.0, 0.25), (0.25, 1.0)]
    assert resolve_bins("float", None, (0, 1)).key_kind == 2         # two numbers for a float column are edges
    assert resolve_bins("float", None, np.array([-np.inf, 0.0, np.inf])).n_bins == 2
    with pytest.raises(ValueError, match="edges"):
        resolve_bins("int", None, None, min_max=lambda: (0, nat.FACET_MAX_BINS))     # one bin too many
    assert resolve_bins("int", None, None, min_max=lambda: (1, nat.FACET_MAX_BINS)).n_bins == nat.FACET_MAX_BINS
    for kind, vocab, bins in (("float", None, None), ("float", None, [0.0]), ("float", None, [0.0, 0.0]), ("float", None, [1.0, 0.5]),
                              ("float", None, [0.0, float("nan")]), ("float", None, [1.0, 1.0 + 1e-12]), ("int", None, [0.5, 1.5]),
                              ("int", None, (3, 2)), ("int", None, [0, 1 << 31]), ("int", None, (0, 1 << 31)), ("int", None, "ab"),
                              ("int", None, 7), ("int", None, None), ("cat", ["a"], [0, 1, 2]), ("cat", [], None),
                              ("int", None, (0, nat.FACET_MAX_BINS)), ("float", None, ["a", "b"]), ("bool", None, None)):
        with pytest.raises(ValueError):
            resolve_bins(kind, vocab, bins)


def test_check_lists():
    from dewi.facets import check_lists
    li, ro = check_lists([0, 2, 2, 3], [5, 5, 0], 6)
    assert li.dtype == np.int64 and ro.tolist() == [5, 5, 0]
    for lims, rows in (([0, 2], [0, 6]), ([0, 2], [-1, 0]), ([1, 2], [0, 1]), ([0, 1], [0, 1]), ([0, 2, 1, 2], [0, 1]), ([0], []),
                       ([0, 1], [0.5])):
        with pytest.raises(ValueError):
            check_lists(lims, rows, 6)


# ------------------------------------------------------------------------------------------ the library, without a device
@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_symbols_are_declared_listed_and_exported(lib):
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    declared = set(re.findall(r"^(?:int|size_t|const char\*)\s+(dewi_\w+)\(", header, flags=re.M))
    assert NEW <= declared and declared == set(nat.EXPORTED_SYMBOLS)
    for name in NEW:
        assert hasattr(lib, name)
    for word in ("DEWI_FACET_MAX_BINS (1 << 20)", "DEWI_FACET_MAX_SELECTIONS 4096", "DEWI_FACET_MAX_SLOTS (1 << 27)"):
        assert word in header
    assert (nat.FACET_MAX_BINS, nat.FACET_MAX_SELECTIONS, nat.FACET_MAX_SLOTS) == (fm.MAX_BINS, fm.MAX_SELECTIONS, fm.MAX_SLOTS)
    notes = (REPO / "INTEGRATION.md").read_text()
    for name in NEW:
        assert name in notes


def test_plan_paths_and_limits(lib):
    from dewi import _native as nat
    try:
        lib.dewi_facet_tuning_set(-1, 0)
        # path 0 while the counters of ONE selection fit 48 KB: 4 bytes per slot, 24 with a value column
        assert nat.facet_plan(1000, 0, 12286, 0, 1, 0)["path"] == 0 and nat.facet_plan(1000, 0, 12287, 0, 1, 0)["path"] == 1
        assert nat.facet_plan(1000, 0, 2046, 1, 3, 2)["path"] == 0 and nat.facet_plan(1000, 0, 2047, 1, 3, 1)["path"] == 1
        p = nat.facet_plan(1 << 20, 0, 1000, 1, 33, 0)
        assert (p["path"], p["per_launch"], p["launches"]) == (0, 12, 3) and p["lds_bytes"] == 12 * 1002 * 4 <= 65536
        # a list element names its selection: all counters in LDS, or none
        assert nat.facet_plan(5000, 0, 1000, 2, 12, 0)["path"] == 0 and nat.facet_plan(5000, 0, 1000, 2, 13, 0)["path"] == 1
        # edges up to 16 KB are staged beside the counters, and a workgroup never asks for more than 64 KB
        assert nat.facet_plan(1000, 2, 4095, 0, 1, 0)["lds_bytes"] == 4096 * 4 + 4097 * 4
        assert nat.facet_plan(1000, 2, 4096, 0, 1, 0)["lds_bytes"] == 4098 * 4
        assert nat.facet_plan(1000, 1, 2046, 0, 1, 2)["lds_bytes"] == 8192 + 2048 * 24 <= 65536
        lib.dewi_facet_tuning_set(1, 3)
        p = nat.facet_plan(1 << 20, 0, 1000, 1, 33, 0)
        assert (p["path"], p["blocks"], p["per_launch"], p["launches"]) == (1, 3, 33, 1)
    finally:
        lib.dewi_facet_tuning_set(-1, 0)


def run(lib, *, keys=1, key_kind=0, n_rows=10, key_lo=0, edges=None, n_bins=4, sel=0, p=1, masks=None, rows=None, lims=None, t=0,
        values=None, vt=0, counts=1, stats=(None, None, None, None), ws=1, ws_bytes=None):
    """``dewi_facet_run`` with 1 standing for a non-null pointer nobody reads: every call here is refused before device work."""
    if ws_bytes is None:
        ws_bytes = int(lib.dewi_facet_workspace_bytes(n_bins, p, vt)) or 256
    buf = (ctypes.c_char * 64)()
    at = ctypes.addressof(buf)
    a = lambda x: None if x is None else at                           # noqa: E731
    return lib.dewi_facet_run(a(keys), key_kind, n_rows, key_lo, a(edges), n_bins, sel, p, a(masks), a(rows), a(lims), t, a(values), vt,
                              a(counts), *[a(s) for s in stats], a(ws), ws_bytes, None)


def test_argument_errors_in_the_stated_order(lib):
    from dewi import _native as nat
    inv, uns, wsp = nat.ERR_INVALID_ARG, nat.ERR_UNSUPPORTED, nat.ERR_WORKSPACE
    full = (1, 1, 1, 1)
    # 1. enums, before a null pointer is looked at
    assert run(lib, key_kind=3, keys=None) == inv and "key_kind" in nat.last_error()
    assert run(lib, sel=-1, keys=None) == inv and "sel_kind" in nat.last_error()
    assert run(lib, vt=3, keys=None) == inv and "value_type" in nat.last_error()
    # 2. pointers, before the sizes
    for kw in ({"keys": None}, {"counts": None}, {"key_kind": 1}, {"key_kind": 2}, {"sel": 1, "p": 2}, {"sel": 2, "lims": 1},
               {"sel": 2, "rows": 1}, {"vt": 1, "stats": full}, {"vt": 2, "values": 1, "stats": (1, 1, None, 1)},
               {"vt": 2, "values": 1, "stats": (None, 1, 1, 1)}):
        assert run(lib, n_rows=-1, **kw) == inv and "null pointer" in nat.last_error(), kw
    # 3. sizes, before the limits
    for kw in ({"n_rows": -1}, {"n_bins": 0}, {"p": 0, "sel": 1, "masks": 1}, {"sel": 2, "rows": 1, "lims": 1, "t": -1}, {"p": 2}):
        assert run(lib, **dict({"n_rows": 1 << 32}, **kw)) == inv, kw
    # 4. limits, before the workspace
    for kw in ({"n_bins": (1 << 20) + 1}, {"p": 4097, "sel": 1, "masks": 1}, {"p": 128, "n_bins": 1 << 20, "sel": 1, "masks": 1},
               {"n_rows": 1 << 32}, {"sel": 2, "rows": 1, "lims": 1, "t": 1 << 32}):
        assert run(lib, ws_bytes=0, **kw) == uns, kw
    # 5. the workspace
    assert run(lib, ws_bytes=255) == wsp and run(lib, ws=None) == wsp
    need = int(lib.dewi_facet_workspace_bytes(1000, 5, 2))
    assert need == 2 * 4 * 5 * 1002 + (-2 * 4 * 5 * 1002) % 256
    assert run(lib, n_bins=1000, p=5, sel=1, masks=1, vt=2, values=1, stats=full, ws_bytes=need - 1) == wsp
    # the size function: 0 for what the call refuses, never 0 otherwise; the limits themselves are served
    assert lib.dewi_facet_workspace_bytes(4, 1, 0) == 256
    for n_bins, p in ((0, 1), ((1 << 20) + 1, 1), (4, 0), (4, 4097), (1 << 20, 128)):
        assert lib.dewi_facet_workspace_bytes(n_bins, p, 0) == 0
    assert lib.dewi_facet_workspace_bytes(4, 1, 3) == 0
    assert lib.dewi_facet_workspace_bytes(1 << 20, 127, 1) > 0 and lib.dewi_facet_workspace_bytes((1 << 15) - 2, 4096, 0) == 256
    assert nat.facet_plan((1 << 32) - 1, 0, 1 << 20, 1, 127, 1)["path"] == 1
    out = (ctypes.c_int64 * 5)()
    assert lib.dewi_facet_plan(1 << 32, 0, 4, 0, 1, 0, out) == uns and lib.dewi_facet_plan(10, 0, 4, 0, 1, 0, None) == inv

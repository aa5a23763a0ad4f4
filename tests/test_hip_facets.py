"""GPU tests of facets: ``dewi_facet_run`` against the NumPy model (``facet_model.py``) — exact, apart from the fp64 sum of fp32
values, which is held to the derived bound ``vcount * 2^-52 * sum|x|`` — and ``facet`` / ``facets`` / ``facet_range`` /
``stratify_by_dewi`` through the index against the model on the same selections.

The C-ABI tests call the library directly, in ``test_hip_where.py``'s habits: the key and value columns are the LAST ``n_rows``
elements of larger buffers whose front holds other values, the column pointers are only 4-byte aligned (a second run: 16-byte
aligned), and every output and the workspace lie between guard bytes (``wsguard``) prefilled with 0xff.  Both paths — counters
in LDS, counters in global memory — run on the same inputs, ``dewi_facet_plan`` pins which one ran.
"""
import ctypes
import itertools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import facet_model as fm
import wsguard as wsg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 37                                   # elements in front of every column: its pointer is 4-byte aligned, no more
GOLDEN = Path(__file__).resolve().parent / "golden" / "facets_stratify.json"
ROWS = [1, 3, 63, 64, 65, 255, 257, 4099, 65537]
LIMIT = {False: 12286, True: 2046}         # the last n_bins whose counters fit LDS: without / with a value column
SELECTIONS = [1, 2, 5, 33]


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    lib = nat.load_library()
    yield lib
    lib.dewi_facet_tuning_set(-1, 0)


class Case:
    """One input of ``dewi_facet_run`` on the host: columns with ``pad`` foreign elements in front, selections, values."""

    def __init__(self, rs, n, n_bins, kind, sel, p, vt, sorted_keys=False, pad=PAD):
        self.n, self.n_bins, self.kind, self.sel, self.vt, self.pad = n, n_bins, kind, sel, vt, pad
        self.p = 1 if sel == fm.SEL_ALL else p
        self.key_lo, self.edges = 0, None
        if kind == fm.KEY_I32_RANGE:
            self.key_lo = int(rs.randint(-50, 50))
            tail = rs.randint(self.key_lo - 2, self.key_lo + n_bins + 2, n).astype(np.int32)
            front = np.full(pad, self.key_lo, dtype=np.int32)
        elif kind == fm.KEY_I32_EDGES:
            self.edges = np.sort(rs.choice(np.arange(-4 * n_bins - 8, 4 * n_bins + 8), n_bins + 1, replace=False)).astype(np.int32)
            tail = rs.randint(int(self.edges[0]) - 3, int(self.edges[-1]) + 4, n).astype(np.int32)
            at = rs.rand(n) < 0.3
            tail[at] = rs.choice(self.edges, int(at.sum()))                       # keys exactly on edges, the last one included
            front = np.full(pad, self.edges[0], dtype=np.int32)
        else:
            e = np.sort(rs.choice(np.arange(-4 * n_bins - 8, 4 * n_bins + 8), n_bins + 1, replace=False)).astype(np.float32) / 8
            if n_bins % 2:
                e[0], e[-1] = -np.inf, np.inf
            if (e == 0).any() and n_bins % 3 == 0:
                e[e == 0] = -0.0
            self.edges = e
            lo, hi = (e[np.isfinite(e)][[0, -1]] if np.isfinite(e).any() else (-1.0, 1.0))
            tail = (rs.uniform(lo - 1, hi + 1, n)).astype(np.float32)
            at = rs.rand(n) < 0.3
            tail[at] = rs.choice(e, int(at.sum()))
            special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
            at = rs.rand(n) < 0.1
            tail[at] = rs.choice(special, int(at.sum()))
            front = np.full(pad, e[1 if n_bins > 1 else 0], dtype=np.float32)
        if sorted_keys:                                                          # a corpus sorted by source: waves of one bin
            tail = tail[np.argsort(fm.slots_of(tail, kind, n_bins, self.key_lo, self.edges), kind="stable")]
        self.keys = np.concatenate([front, tail])
        self.values = None
        if vt == fm.VALUE_I32:
            v = rs.randint(-1000, 1000, pad + n).astype(np.int32)
            v[rs.rand(pad + n) < 0.05] = fm.INT32_MAX
            v[rs.rand(pad + n) < 0.05] = fm.INT32_MIN
            self.values = v
        elif vt == fm.VALUE_F32:
            v = (rs.randn(pad + n) * 10.0 ** rs.randint(-3, 30, pad + n)).astype(np.float32)
            v[rs.rand(pad + n) < 0.1] = np.nan
            v[rs.rand(pad + n) < 0.05] = -0.0
            v[rs.rand(pad + n) < 0.05] = 0.0
            self.values = v
        self.masks = self.rows = self.lims = None
        if sel == fm.SEL_MASKS:
            m = (rs.rand(self.p, n) < rs.uniform(0.2, 0.9)).astype(np.uint8) * rs.randint(1, 256, (self.p, n)).astype(np.uint8)
            if self.p > 1:
                m[1] = 0                                                         # an all-zero mask
            self.masks = m
        elif sel == fm.SEL_LISTS:
            t = int(min(2 * n + 7, 5000))
            self.rows = rs.randint(-3, n + 3, t).astype(np.int64)                # duplicates, and ids on either side of the range
            cuts = np.sort(rs.randint(0, t + 1, self.p - 1))
            self.lims = np.concatenate([[0], cuts, [t]]).astype(np.int64)
            if self.p > 2:
                self.lims[2] = self.lims[1]                                      # an empty segment

    def model(self):
        pad = self.pad
        return fm.facet(self.keys[pad:], self.kind, self.n_bins, self.key_lo, self.edges, self.sel, self.masks, self.rows, self.lims,
                        None if self.values is None else self.values[pad:])

    def t(self):
        return 0 if self.rows is None else len(self.rows)


def run(lib, c, prefill="0xff", force_path=-1, max_blocks=0, ws_prefill=None):
    """``dewi_facet_run`` on a ``Case`` -> (host outputs like the model's, the plan that ran)."""
    from dewi import _native as nat
    torch.cuda.set_device(0)
    lib.dewi_facet_tuning_set(force_path, max_blocks)
    try:
        plan = nat.facet_plan(c.t() if c.sel == fm.SEL_LISTS else c.n, c.kind, c.n_bins, c.sel, c.p, c.vt)
        slots = c.p * (c.n_bins + 2)
        keys = torch.from_numpy(c.keys).to(DEV)
        edges = None if c.edges is None else torch.from_numpy(c.edges).to(DEV)
        values = None if c.values is None else torch.from_numpy(c.values).to(DEV)
        masks = None if c.masks is None else torch.from_numpy(np.ascontiguousarray(c.masks)).to(DEV)
        rows = None if c.rows is None else torch.from_numpy(c.rows if len(c.rows) else np.zeros(1, np.int64)).to(DEV)
        lims = None if c.lims is None else torch.from_numpy(c.lims).to(DEV)
        need = int(lib.dewi_facet_workspace_bytes(c.n_bins, c.p, c.vt))
        assert need >= 256
        ws = wsg.GuardedBuffer(need, DEV, ws_prefill or prefill, label="workspace")
        out = {"counts": wsg.GuardedBuffer(slots * 8, DEV, prefill, label="d_counts")}
        if c.vt:
            out.update(vcount=wsg.GuardedBuffer(slots * 8, DEV, prefill, label="d_vcount"),
                       vmin=wsg.GuardedBuffer(slots * 4, DEV, prefill, label="d_vmin"),
                       vmax=wsg.GuardedBuffer(slots * 4, DEV, prefill, label="d_vmax"),
                       vsum=wsg.GuardedBuffer(slots * 8, DEV, prefill, label="d_vsum"))
        p_ = lambda name: out[name].view.data_ptr() if name in out else None     # noqa: E731
        nat.check(lib.dewi_facet_run(
            keys.data_ptr() + 4 * c.pad, c.kind, c.n, c.key_lo, None if edges is None else edges.data_ptr(), c.n_bins, c.sel, c.p,
            None if masks is None else masks.data_ptr(), None if rows is None else rows.data_ptr(),
            None if lims is None else lims.data_ptr(), c.t(), None if values is None else values.data_ptr() + 4 * c.pad, c.vt,
            p_("counts"), p_("vcount"), p_("vmin"), p_("vmax"), p_("vsum"), ws.view.data_ptr(), need,
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        ws.check(interior=False)
        got = {}
        for name, buf in out.items():
            buf.check(interior=False)                                            # the guards around every output are untouched
            dtype = {"counts": np.int64, "vcount": np.int64, "vsum": np.float64 if c.vt == fm.VALUE_F32 else np.int64}.get(
                name, np.float32 if c.vt == fm.VALUE_F32 else np.int32)
            got[name] = buf.view.cpu().numpy().view(dtype).reshape(c.p, c.n_bins + 2).copy()
        return got, plan
    finally:
        lib.dewi_facet_tuning_set(-1, 0)


def assert_equals_model(got, want, what):
    assert np.array_equal(got["counts"], want["counts"]), (what, "counts")
    if "vcount" not in want:
        assert set(got) == {"counts"}
        return
    assert np.array_equal(got["vcount"], want["vcount"]), (what, "vcount")
    for name in ("vmin", "vmax"):                                                # bit for bit: -0 is not +0 here
        assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), (what, name)
    if want["vsum"].dtype == np.int64:
        assert np.array_equal(got["vsum"], want["vsum"]), (what, "vsum")
    else:
        err, bound = np.abs(got["vsum"] - want["vsum"]), fm.sum_bound(want["vcount"], want["vabs"])
        assert np.all(err <= bound), (what, "vsum", float(err.max()), float(bound[np.argmax(err - bound)]))
        assert np.all(got["vsum"][want["vcount"] == 0] == 0.0), (what, "vsum of empty slots")


def schedule():
    """[(n, n_bins, kind, sel, p, vt, sorted)]: every n_rows with every n_bins, the other axes rotating so that over the sweep
    every (selection form, key kind, value type) and every P meet small and large n, few and many bins, both paths."""
    combos = list(itertools.product((fm.SEL_ALL, fm.SEL_MASKS, fm.SEL_LISTS), (0, 1, 2), (0, 1, 2)))
    out, i = [], 0
    for j, n in enumerate(ROWS):
        for b in (1, 2, 63, 64, 65, 1000, "limit", "limit+1", 70001):
            sel, kind, vt = combos[(7 * i + j) % len(combos)]
            n_bins = LIMIT[vt != 0] + (b == "limit+1") if isinstance(b, str) else b
            p = SELECTIONS[(i // 3) % 4]
            if n_bins > 12287:
                p = min(p, 5)                                                    # (keeps the largest outputs at a few MB)
            out.append((n, n_bins, kind, sel, p, vt, i % 2 == 1))
            i += 1
    have = {(c[3], c[2], c[5]) for c in out}
    out += [(4099, 300, kind, sel, 5, vt, True) for sel, kind, vt in combos if (sel, kind, vt) not in have]   # what the rotation missed
    return out


def test_the_sweep_covers_what_it_claims():
    from dewi import _native as nat
    s = schedule()
    assert {(c[3], c[2], c[5]) for c in s} == set(itertools.product((0, 1, 2), (0, 1, 2), (0, 1, 2)))
    for sel in (fm.SEL_MASKS, fm.SEL_LISTS):
        assert {c[4] for c in s if c[3] == sel} == set(SELECTIONS)
    for vt in (0, 1, 2):
        assert nat.facet_plan(100, 0, LIMIT[vt != 0], 0, 1, vt)["path"] == 0 and nat.facet_plan(100, 0, LIMIT[vt != 0] + 1, 0, 1, vt)["path"] == 1
        assert {c[1] for c in s if c[5] == vt} >= {LIMIT[vt != 0], LIMIT[vt != 0] + 1}
    assert {c[1] for c in s} >= {1, 2, 63, 64, 65, 1000, 70001}


# ------------------------------------------------------------------------------------------------------- 1. the ABI sweep
@pytest.mark.parametrize("n", ROWS)
def test_abi_sweep_equals_the_model_on_both_paths(lib, n):
    paths = set()
    for _, n_bins, kind, sel, p, vt, srt in [c for c in schedule() if c[0] == n]:
        rs = np.random.RandomState(n * 7 + n_bins)
        c = Case(rs, n, n_bins, kind, sel, p, vt, sorted_keys=srt)
        what = (n, n_bins, kind, sel, c.p, vt)
        want = c.model()
        got, plan = run(lib, c)
        assert_equals_model(got, want, what + ("auto", plan["path"]))
        paths.add(plan["path"])
        # the other path on the same inputs (where the counters fit LDS at all), and several workgroups and trips
        forced, fplan = run(lib, c, force_path=1, max_blocks=3, prefill="random")
        assert fplan["path"] == 1 and fplan["blocks"] <= 3
        assert_equals_model(forced, want, what + ("forced", 1))
        if plan["path"] == 0 and n >= 4099:
            small, splan = run(lib, c, max_blocks=2, prefill="zeros")
            assert splan["path"] == 0 and splan["blocks"] == 2
            assert_equals_model(small, want, what + ("two workgroups", 0))
    assert paths == {0, 1}


def test_aligned_columns_take_the_wide_loads(lib):
    """The same rows behind a front of 32 elements: 16-byte aligned columns (the sweep: 4-byte aligned, no more)."""
    for n, vt, sel in ((4099, fm.VALUE_F32, fm.SEL_MASKS), (65537, fm.VALUE_I32, fm.SEL_ALL), (257, fm.VALUE_NONE, fm.SEL_MASKS)):
        c = Case(np.random.RandomState(n), n, 100, fm.KEY_F32_EDGES, sel, 5, vt, pad=32)
        want = c.model()
        for force in (-1, 1):
            got, _ = run(lib, c, force_path=force)
            assert_equals_model(got, want, (n, vt, sel, force))


def test_more_rows_than_one_trip_of_the_grid(lib):
    n = 2_200_003                                                                # 512 workgroups of 1024 rows: five trips
    c = Case(np.random.RandomState(5), n, 1000, fm.KEY_I32_RANGE, fm.SEL_MASKS, 2, fm.VALUE_I32, sorted_keys=True)
    want = c.model()
    got, plan = run(lib, c)
    assert plan == {"path": 0, "blocks": 512, "per_launch": 2, "lds_bytes": 2 * 1002 * 24, "launches": 1}
    assert_equals_model(got, want, "grid-stride")
    assert want["counts"][0, :1000].min() > 0


# ------------------------------------------------------------------------------------------------------- 2. hard inputs
@pytest.mark.parametrize("vt", [fm.VALUE_NONE, fm.VALUE_I32, fm.VALUE_F32])
@pytest.mark.parametrize("force", [-1, 1])
def test_every_row_in_one_bin(lib, vt, force):
    c = Case(np.random.RandomState(1), 70_001, 1000, fm.KEY_I32_RANGE, fm.SEL_MASKS, 2, vt)
    c.keys[:] = c.key_lo + 417
    c.masks[1] = 1
    want = c.model()
    got, plan = run(lib, c, force_path=force)
    assert plan["path"] == (1 if force == 1 else 0)
    assert_equals_model(got, want, ("one bin", vt, force))
    assert got["counts"][1, 417] == 70_001 and got["counts"][1].sum() == 70_001


@pytest.mark.parametrize("key_lo", [fm.INT32_MIN, fm.INT32_MAX, -1, 0])
def test_keys_at_the_int32_extremes(lib, key_lo):
    c = Case(np.random.RandomState(2), 1000, 3, fm.KEY_I32_RANGE, fm.SEL_ALL, 1, fm.VALUE_I32)
    c.key_lo = key_lo
    c.keys[c.pad:] = np.random.RandomState(3).choice(
        np.array([fm.INT32_MIN, fm.INT32_MIN + 1, fm.INT32_MIN + 2, -1, 0, 1, fm.INT32_MAX - 2, fm.INT32_MAX - 1, fm.INT32_MAX], dtype=np.int32), 1000)
    want = c.model()
    for force in (-1, 1):
        got, _ = run(lib, c, force_path=force)
        assert_equals_model(got, want, ("extremes", key_lo, force))
    if key_lo == fm.INT32_MAX:                                                   # INT32_MIN - INT32_MAX does not wrap into bin 1
        assert got["counts"][0].tolist() == [int((c.keys[c.pad:] == fm.INT32_MAX).sum()), 0, 0, 1000 - int((c.keys[c.pad:] == fm.INT32_MAX).sum()), 0]


def test_a_value_column_that_is_all_nan(lib):
    c = Case(np.random.RandomState(4), 4099, 7, fm.KEY_F32_EDGES, fm.SEL_MASKS, 3, fm.VALUE_F32)
    c.values[:] = np.nan
    want = c.model()
    for force in (-1, 1):
        got, _ = run(lib, c, force_path=force)
        assert_equals_model(got, want, ("all NaN", force))
        assert got["vcount"].sum() == 0 and np.all(got["vmin"] == np.inf) and np.all(got["vmax"] == -np.inf) and np.all(got["vsum"] == 0.0)
        assert got["counts"].sum() == int((c.masks != 0).sum()) and got["counts"][:, -1].sum() > 0      # NaN KEYS are counted


def test_lists_with_duplicates_empty_and_out_of_range_segments(lib):
    n = 300
    c = Case(np.random.RandomState(6), n, 5, fm.KEY_I32_EDGES, fm.SEL_LISTS, 5, fm.VALUE_F32)
    segs = [[7] * 130 + [8, 8, 9], [], [-1, -5, n, n + 1, 1 << 40, -(1 << 40)] * 20, list(range(n)) * 2, [n - 1]]
    c.rows = np.array(sum(segs, []), dtype=np.int64)
    c.lims = np.cumsum([0] + [len(s) for s in segs]).astype(np.int64)
    want = c.model()
    assert want["counts"].sum(axis=1).tolist() == [133, 0, 0, 2 * n, 1]
    for force in (-1, 1):
        got, plan = run(lib, c, force_path=force, max_blocks=2)
        assert plan["path"] == (1 if force == 1 else 0)
        assert_equals_model(got, want, ("lists", force))
    # nothing listed at all: cleared outputs
    c.rows, c.lims = np.zeros(0, np.int64), np.zeros(6, np.int64)
    got, _ = run(lib, c)
    assert_equals_model(got, c.model(), "T == 0")
    assert got["counts"].sum() == 0 and np.all(got["vmin"] == np.inf)


def test_an_all_zero_mask_and_no_rows(lib):
    c = Case(np.random.RandomState(8), 257, 64, fm.KEY_I32_RANGE, fm.SEL_MASKS, 2, fm.VALUE_I32)
    c.masks[:] = 0
    got, _ = run(lib, c)
    assert_equals_model(got, c.model(), "zero masks")
    assert got["counts"].sum() == 0 and np.all(got["vmin"] == fm.INT32_MAX) and np.all(got["vmax"] == fm.INT32_MIN) and got["vsum"].sum() == 0


# ------------------------------------------------------------------------------------------------------- 3. garbage on entry
def test_workspace_and_outputs_holding_garbage_change_nothing(lib):
    c = Case(np.random.RandomState(9), 4099, 300, fm.KEY_F32_EDGES, fm.SEL_MASKS, 5, fm.VALUE_I32)
    want = c.model()
    for force in (-1, 1):
        runs = [run(lib, c, prefill=f, ws_prefill=w, force_path=force)[0]
                for f, w in (("zeros", "zeros"), ("0xff", "random"), ("random", "0x7f"), ("0x7f", "0xff"))]
        for r in runs:
            assert_equals_model(r, want, ("garbage", force))
            for name in r:
                assert r[name].tobytes() == runs[0][name].tobytes(), name        # int values: every output is exact


# ------------------------------------------------------------------------------------------------------- 4. through the index
N, D = 5000, 32
_world = {}


def world():
    """The corpus (its ``dewi`` payload is the golden fixture's), its attributes on the host, two indexes — built once."""
    if _world:
        return _world
    import dewi_oracle as orc
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.types import payloads_from_columns
    with open(GOLDEN) as fh:
        g = json.load(fh)
    rs = np.random.RandomState(33)
    raw = orc.synth_corpus(N, D, seed=9)
    pay = dict(orc.synth_payload_columns(N, seed=9))
    pay["dewi"] = np.asarray(g["dewi_times_64"], dtype=np.float64) / 64.0
    ids = [f"doc_{i:05d}" for i in range(N)]
    sites = [f"site{j:02d}.org" for j in range(30)]
    site = [None if rs.rand() < 0.05 else sites[min(int(i * 30 / N + rs.randint(0, 2)), 29)] for i in range(N)]   # nearly sorted by source
    score = rs.randn(N)
    score[rs.rand(N) < 0.1] = np.nan
    attrs = {"site": site, "year": rs.randint(1990, 2026, N).astype(np.int64), "score": score}
    plist = payloads_from_columns(pay)
    exact = ExactIndex(dim=D)
    exact.add_batch(ids, raw, plist)
    facade = DewiIndex(dim=D, use_ann=False)
    facade.add_batch(ids, raw, plist)
    for ix in (exact, facade):
        ix.build()
        ix.set_attributes(**attrs)
        ix.attributes_from_payload("dewi")
    vocab = sorted(set(s for s in site if s is not None))
    code = {s: i for i, s in enumerate(vocab)}
    host = {"site": np.array([-1 if s is None else code[s] for s in site], dtype=np.int32), "year": attrs["year"].astype(np.int32),
            "score": score.astype(np.float32), "dewi": pay["dewi"].astype(np.float32)}
    _world.update(raw=raw, pay=pay, plist=plist, ids=ids, attrs=attrs, host=host, vocab=vocab, exact=exact, facade=facade, golden=g,
                  Q=orc.synth_queries(5, D, seed=3))
    return _world


def model_facet(w, column, mask=None, rows=None, lims=None, bins=None, value=None, host=None):
    """The model's answer for an index call: (keys, counts [P, n_bins], other [P], nan [P], stats of the model or None)."""
    from dewi.facets import resolve_bins
    host = host or w["host"]
    col = host[column]
    kind = "cat" if column == "site" else ("float" if col.dtype == np.float32 else "int")
    fb = resolve_bins(kind, w["vocab"] if kind == "cat" else None, bins, column, lambda: (int(col.min()), int(col.max())))
    sel = fm.SEL_ALL if mask is None and rows is None else (fm.SEL_MASKS if rows is None else fm.SEL_LISTS)
    m = fm.facet(col, fb.key_kind, fb.n_bins, fb.key_lo, fb.edges, sel, None if mask is None else np.atleast_2d(mask).astype(np.uint8),
                 rows, lims, None if value is None else host[value])
    return fb, m


def assert_facet(f, fb, m, p=0):
    n = fb.n_bins
    assert f.keys == fb.keys and f.counts.tolist() == m["counts"][p, :n].tolist()
    assert (f.other, f.nan, f.total) == (int(m["counts"][p, n]), int(m["counts"][p, n + 1]), int(m["counts"][p].sum()))
    if "vcount" not in m:
        assert f.stats is None
        return
    assert f.stats["count"].tolist() == m["vcount"][p, :n].tolist()
    assert f.stats["min"].tobytes() == m["vmin"][p, :n].tobytes() and f.stats["max"].tobytes() == m["vmax"][p, :n].tobytes()
    if m["vsum"].dtype == np.int64:
        assert f.stats["sum"].tolist() == m["vsum"][p, :n].tolist()
    else:
        assert np.all(np.abs(f.stats["sum"] - m["vsum"][p, :n]) <= fm.sum_bound(m["vcount"][p, :n], m["vabs"][p, :n]))
    empty = m["vcount"][p, :n] == 0
    assert np.isnan(f.stats["mean"][empty]).all() and not np.isnan(f.stats["mean"][~empty]).any()
    with np.errstate(invalid="ignore"):
        assert np.allclose(f.stats["mean"][~empty], f.stats["sum"][~empty] / f.stats["count"][~empty], rtol=0, atol=0)


def test_facet_under_every_filter_form_equals_the_model():
    from dewi.where import col
    w = world()
    rs = np.random.RandomState(1)
    mask = rs.rand(N) < 0.3
    rows = np.flatnonzero(mask)
    where = (col("year") >= 2010) & (col("site") != "site03.org")
    wmask = (w["host"]["year"] >= 2010) & (w["host"]["site"] != w["vocab"].index("site03.org"))
    for ix in (w["exact"], w["facade"]):
        forms = [(None, None), (mask, mask), (torch.from_numpy(mask).to(DEV), mask), ([w["ids"][r] for r in rows], mask), (rows, mask),
                 (ix.make_filter(mask), mask), (where, wmask), (ix.make_filter_where(where), wmask)]
        for given, truth in forms:
            for column, bins, value in (("site", None, "score"), ("year", None, None), ("year", (2000, 2009), "year"),
                                        ("year", [1990, 2000, 2010, 2025], "score"), ("score", [-np.inf, -1.0, 0.0, 1.0, np.inf], "year"),
                                        ("dewi", [0.0, 0.25, 0.5, 0.75, 1.0], None)):
                fb, m = model_facet(w, column, mask=truth, bins=bins, value=value)
                got = ix.facet(column, filter=given, bins=bins, value=value)
                assert_facet(got, fb, m)
    f = w["facade"].facet("site", filter=where)
    assert f.keys == w["vocab"] and f.other == int((wmask & (w["host"]["site"] < 0)).sum()) and f.total == int(wmask.sum())
    assert f.top(3) == sorted(zip(f.keys, f.counts.tolist()), key=lambda kc: (-kc[1], kc[0]))[:3]
    assert abs(sum(f.proportions().values()) + f.other / f.total - 1.0) < 1e-12


def test_group_labels_as_keys():
    w = world()
    labels = np.arange(N) % 11 - 1                                               # -1: ungrouped, counted as other
    for ix in (w["exact"], w["facade"]):
        f = ix.facet(ix.make_groups(labels))
        assert f.keys == list(range(10)) and f.counts.tolist() == np.bincount(labels[labels >= 0], minlength=10).tolist()
        assert f.other == int((labels < 0).sum()) and f.nan == 0


def test_a_list_of_33_predicates_equals_33_single_calls_and_a_2d_mask():
    from dewi.where import col
    w = world()
    ix = w["facade"]
    wheres = [(col("year") >= 1990 + j) & (col("score") < 2.0 - 0.1 * j) for j in range(33)]
    many = ix.facet("site", filter=wheres, value="score")
    assert isinstance(many, list) and len(many) == 33
    host = w["host"]
    with np.errstate(invalid="ignore"):
        masks = np.stack([(host["year"] >= 1990 + j) & (host["score"] < np.float32(2.0 - 0.1 * j)) for j in range(33)])
    fb, m = model_facet(w, "site", mask=masks, value="score")
    for j in (0, 7, 32):
        one = ix.facet("site", filter=wheres[j], value="score")
        assert one.counts.tolist() == many[j].counts.tolist() and (one.other, one.nan) == (many[j].other, many[j].nan)
        for name in ("count", "min", "max"):
            assert one.stats[name].tobytes() == many[j].stats[name].tobytes()
    for j in range(33):
        assert_facet(many[j], fb, m, j)
    two_d = ix.facet("site", filter=masks, value="score")
    for j in range(33):
        assert_facet(two_d[j], fb, m, j)


def test_facets_equals_the_per_column_calls():
    from dewi.where import col
    w = world()
    ix = w["facade"]
    where = col("score") > 0.0
    bins = {"score": [-3.0, 0.0, 0.5, 3.0], "year": (1995, 2020)}
    got = ix.facets(["site", "year", "score"], filter=where, bins=bins)
    assert list(got) == ["site", "year", "score"]
    for name, f in got.items():
        one = ix.facet(name, filter=where, bins=bins.get(name))
        assert f.as_dict() == one.as_dict()
    both = ix.facets(["site", "year"], filter=[where, ~where])
    assert [f.total for f in both["site"]] == [int(ix.count_where(where)), int(ix.count_where(~where))]
    with pytest.raises(ValueError):
        ix.facets(["site"], bins={"year": (0, 1)})


def test_facet_range_equals_range_search_plus_the_model():
    w = world()
    Q = w["Q"].copy()
    Q[1] = w["raw"][17]                                                          # a query with a certain hit
    thr = np.array([0.1, 0.9, 0.0, 2.0, 0.2], dtype=np.float32)                  # query 3: no cosine reaches 2
    for ix, backend in ((w["exact"], w["exact"]), (w["facade"], w["facade"]._backend)):
        lims, rows, _, _ = backend.range_search_batch(Q, thr, sort=False)
        assert lims[4] == lims[3] and lims[2] > lims[1] and lims[-1] == len(rows) > 0
        fb, m = model_facet(w, "site", rows=rows, lims=lims, value="score")
        got = ix.facet_range(Q, thr, "site", value="score")
        assert len(got) == 5 and got[3].total == 0
        for j in range(5):
            assert_facet(got[j], fb, m, j)
        mask = np.arange(N) % 3 == 0
        lims, rows, _, _ = backend.range_search_batch(Q, thr, filter=mask, sort=False)
        fb, m = model_facet(w, "year", rows=rows, lims=lims, bins=(1990, 2025))
        got = ix.facet_range(Q, thr, "year", filter=mask, bins=(1990, 2025))
        for j in range(5):
            assert_facet(got[j], fb, m, j)
    # the same through rows=: host arrays and device tensors
    lims, rows, _, _ = w["exact"].range_search_batch(Q, thr, sort=False)
    for given in ((lims, rows), (torch.from_numpy(lims).to(DEV), torch.from_numpy(rows).to(DEV))):
        got = w["facade"].facet("year", rows=given)
        fb, m = model_facet(w, "year", rows=rows, lims=lims)
        for j in range(5):
            assert_facet(got[j], fb, m, j)


def test_argument_errors_of_the_index_methods():
    w = world()
    ix = w["facade"]
    with pytest.raises(ValueError):
        ix.facet("year", rows=([0, 1], [N]))                                    # an id out of range
    with pytest.raises(ValueError):
        ix.facet("year", rows=(torch.tensor([0, 1]).to(DEV), torch.tensor([-1]).to(DEV)))
    with pytest.raises(ValueError):
        ix.facet("year", rows=([0, 1], [0]), filter=np.ones(N, bool))
    with pytest.raises(ValueError):
        ix.facet("nope")
    with pytest.raises(ValueError):
        ix.facet("score")                                                        # a float column needs edges
    with pytest.raises(ValueError):
        ix.facet("year", value="site")
    with pytest.raises(NotImplementedError):
        ix.facet_range(w["Q"], 0.5, "site", filter=np.ones((5, N), bool))


def test_stratify_by_dewi_equals_the_golden_fixture():
    from dewi.backends import ExactIndex
    w = world()
    for ix in (w["exact"], w["facade"]):
        for c in w["golden"]["cases"]:
            lims = np.cumsum([0] + [len(s) for s in c["segments"]]).astype(np.int64)
            rows = np.asarray(sum(c["segments"], []), dtype=np.int64)
            want = {(lo, hi): v for lo, hi, v in c["expected"]}
            assert ix.stratify_by_dewi(c["bins"], rows=(lims, rows)) == want, c["name"]
        all_case = next(c for c in w["golden"]["cases"] if c["name"] == "all")
        assert ix.stratify_by_dewi(all_case["bins"]) == {(lo, hi): v for lo, hi, v in all_case["expected"]}
        mask = np.arange(N) < 2500
        got = ix.stratify_by_dewi([0.25, 0.5], filter=mask)
        d = w["host"]["dewi"][:2500]
        assert got == {(0.25, 0.5): int(((d >= 0.25) & (d <= 0.5)).sum()) / 2500}
        with pytest.raises(ValueError):
            ix.stratify_by_dewi([0.5])
    bare = ExactIndex(dim=D)
    bare.add_batch(w["ids"][:50], w["raw"][:50], w["plist"][:50])
    with pytest.raises(ValueError, match="attributes_from_payload"):
        bare.stratify_by_dewi([0.0, 1.0])


def test_facets_after_remove_and_upsert_equal_a_fresh_index_and_round_trip_files(tmp_path):
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.where import col
    w = world()
    rs = np.random.RandomState(12)
    n0 = 2000
    ids, raw, plist, attrs = w["ids"], w["raw"], w["plist"], w["attrs"]
    ix = DewiIndex(dim=D, use_ann=False)
    ix.add_batch(ids[:n0], raw[:n0], plist[:n0])
    ix.build()
    ix.set_attributes(site=attrs["site"][:n0], year=attrs["year"][:n0], score=attrs["score"][:n0])
    ix.attributes_from_payload("dewi")
    stale = ix.make_filter(np.arange(n0) % 2 == 0)
    gone = [ids[i] for i in rs.choice(n0, 150, replace=False)]
    ix.remove(gone)
    new = list(range(n0, n0 + 80))
    ix.reserve(2200)
    ix.upsert_batch([ids[i] for i in new], raw[new], [plist[i] for i in new])
    ix.update_attributes([ids[i] for i in new], site=[attrs["site"][i] for i in new], year=attrs["year"][new], score=attrs["score"][new])
    with pytest.raises(ValueError):
        ix.facet("site", filter=stale)                                           # a stale prepared filter raises, as everywhere
    order = list(ix._backend._doc_ids)
    at = [int(d[4:]) for d in order]
    fresh = ExactIndex(dim=D)
    fresh.add_batch(order, raw[at], [plist[i] for i in at])
    fresh.build()
    fresh.set_attributes(site=[attrs["site"][i] for i in at], year=attrs["year"][at], score=attrs["score"][at])
    fresh.attributes_from_payload("dewi")
    where = (col("year") < 2015) | col("score").isnan()
    calls = (("site", None, "score"), ("year", None, None), ("score", [-2.0, 0.0, 2.0], "year"), ("dewi", [0.0, 0.5, 1.0], None))
    for column, bins, value in calls:
        for flt in (None, where):
            a, b = ix.facet(column, filter=flt, bins=bins, value=value), fresh.facet(column, filter=flt, bins=bins, value=value)
            assert a.keys == b.keys and a.counts.tolist() == b.counts.tolist() and (a.other, a.nan, a.total) == (b.other, b.nan, b.total)
            if value == "year":
                assert a.as_dict() == b.as_dict()
    assert ix.facet("year").total == len(order) == n0 - 150 + 80
    ix.save(tmp_path / "ix")
    back = DewiIndex.load(tmp_path / "ix")
    for column, bins, value in calls:
        a, b = ix.facet(column, filter=where, bins=bins, value=value), back.facet(column, filter=where, bins=bins, value=value)
        assert a.keys == b.keys and a.counts.tolist() == b.counts.tolist() and (a.other, a.nan) == (b.other, b.nan)
        if value is not None:
            for name in ("count", "min", "max"):
                assert a.stats[name].tobytes() == b.stats[name].tobytes()
    assert back.stratify_by_dewi([0.0, 0.5, 1.0]) == ix.stratify_by_dewi([0.0, 0.5, 1.0])

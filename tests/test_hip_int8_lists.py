"""GPU, through the raw ABI: the int8 scan over allow-lists, per-query lists and IVF probe buffers (csrc/knn_scan_i8.hip, the
LIST / QMASK kernels) against tests/int8_list_model.py.

The int8 scores are integer arithmetic, so the records are compared BIT FOR BIT: ids, sim bits, order, padding and the payload
pair.  The model is fed the library's own prepared queries and the library's own codes (both pinned by tests/test_hip_int8.py);
every workspace has exactly the required size.

Shapes: both geometries — rows of 1, 3 (a masked lane) and 32 units; rows of 33 .. 256 units with every units-per-lane count
and every rows-in-flight choice the launcher instantiates (528: 1 x 12, 768: 1 x 8, 1040: 2 x 6, 1280: 2 x 4, 1536: 2 x 3,
2064: 3 x 2, 3104: 4 x 2, 4096: 4 x 1) —, lists shorter than the rows in flight, more than one workgroup (4 099 rows), the
three list forms (c <= 64, c <= 256, dense), passes of four queries plus singles, and the second query word (37 queries).
"""
import ctypes

import numpy as np
import pytest

import int8_list_model as lm
import int8_model as im
import wsguard
from test_hip_int8 import (assert_records_equal, candidates_dev, corpus_rows, payload, prepare_dev, quantize_dev, same_bits)

pytestmark = pytest.mark.gpu

_cache = {}


def _lib():
    from dewi import _native as nat
    return nat.load_library()


class Setup:
    """One quantised corpus on the device and on the host."""

    def __init__(self, dim, n, kind="gauss"):
        import torch
        self.dim, self.n = dim, n
        self.x = corpus_rows(kind, n, dim, 31 * dim + n)
        self.dewi, self.ent = payload(n, dim)
        self.E_dev = torch.from_numpy(self.x).cuda()
        self.codes, self.scales = quantize_dev(self.E_dev)
        self.dewi_dev, self.ent_dev = torch.from_numpy(self.dewi).cuda(), torch.from_numpy(self.ent).cuda()
        self.rc, self.rsc = self.codes.cpu().numpy(), self.scales.cpu().numpy()


def setup(dim, n, kind="gauss"):
    key = (dim, n, kind)
    if key not in _cache:
        if len(_cache) > 6:
            _cache.clear()
        _cache[key] = Setup(dim, n, kind)
    return _cache[key]


def queries(S, b, seed, first=0):
    import torch
    q = np.random.RandomState(seed).randn(b, S.dim).astype(np.float32)
    q[0] = S.x[first]
    Q_dev = torch.from_numpy(q).cuda()
    qc, qs, _ = prepare_dev(Q_dev)
    return Q_dev, qc, qs


def filter_dev(mask, dim):
    """``dewi_filter_prepare`` (elem_type 0) -> (buffer, n_allowed)."""
    import torch
    from dewi import _native as nat
    lib, n = _lib(), int(mask.shape[0])
    need = int(lib.dewi_filter_bytes(n, dim, 0))
    buf = torch.empty(need, dtype=torch.uint8, device="cuda")
    m8 = torch.from_numpy(np.ascontiguousarray(mask).view(np.uint8)).cuda()
    n_a = ctypes.c_int64(0)
    nat.check(lib.dewi_filter_prepare(0, n, dim, nat.ptr(m8), nat.ptr(buf), need, ctypes.byref(n_a), nat.stream_ptr()))
    assert n_a.value == int(mask.sum())
    return buf, n_a.value


def query_filter_dev(masks, dim):
    """``dewi_query_filter_prepare`` (elem_type 0) -> (buffer, n_union, counts)."""
    import torch
    from dewi import _native as nat
    lib = _lib()
    b, n = masks.shape
    need = int(lib.dewi_query_filter_bytes(n, dim, 0, b))
    buf = torch.empty(need, dtype=torch.uint8, device="cuda")
    m8 = torch.from_numpy(np.ascontiguousarray(masks).view(np.uint8)).cuda()
    n_u = ctypes.c_int64(0)
    counts = (ctypes.c_int64 * b)()
    nat.check(lib.dewi_query_filter_prepare(0, n, dim, b, nat.ptr(m8), nat.ptr(buf), need, ctypes.byref(n_u), counts, nat.stream_ptr()))
    assert list(counts) == masks.sum(axis=1).tolist() and n_u.value == int(masks.any(axis=0).sum())
    return buf, n_u.value, list(counts)


def workspace(n_scan, dim, b, c, ws):
    import torch
    need = int(_lib().dewi_knn_i8_filtered_workspace_bytes(n_scan, dim, b, c))
    assert need > 0
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device="cuda"), need
    assert ws.numel() == need
    return ws, need


def one_list_dev(S, Q_dev, c, buf, n_a, id_offset=0, ws=None, out=None, codes=None, scales=None):
    """``dewi_knn_candidates_i8_filtered`` in a workspace of exactly the required size -> records [B, c] on the host."""
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    b = int(Q_dev.shape[0])
    ws, need = workspace(n_a, S.dim, b, c, ws)
    if out is None:
        out = torch.empty((b, c, 4), dtype=torch.int32, device="cuda")
    nat.check(_lib().dewi_knn_candidates_i8_filtered(
        nat.ptr(S.codes if codes is None else codes), nat.ptr(S.scales if scales is None else scales), S.n, S.dim, nat.ptr(buf), n_a,
        nat.ptr(Q_dev), b, nat.ptr(S.dewi_dev), nat.ptr(S.ent_dev), c, id_offset, nat.ptr(out), nat.ptr(ws), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    return records_to_numpy(out)


def per_query_dev(S, Q_dev, c, buf, n_u, counts, id_offset=0, ws=None, out=None):
    """``dewi_knn_candidates_i8_query_filtered`` in a workspace of exactly the required size -> records [B, c] on the host."""
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    b = int(Q_dev.shape[0])
    ws, need = workspace(n_u, S.dim, b, c, ws)
    if out is None:
        out = torch.empty((b, c, 4), dtype=torch.int32, device="cuda")
    nat.check(_lib().dewi_knn_candidates_i8_query_filtered(
        nat.ptr(S.codes), nat.ptr(S.scales), S.n, S.dim, nat.ptr(buf), n_u, (ctypes.c_int64 * b)(*counts), nat.ptr(Q_dev), b,
        nat.ptr(S.dewi_dev), nat.ptr(S.ent_dev), c, id_offset, nat.ptr(out), nat.ptr(ws), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    return records_to_numpy(out)


def list_mask(kind, n, seed):
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "one":
        m[n // 3] = True
    elif kind == "five":                      # fewer than the rows in flight
        m[[0, 17, n // 2, n - 2, n - 1]] = True
    elif kind == "second":
        m[1::2] = True
    elif kind == "random":
        m = np.random.RandomState(seed).rand(n) < 0.3
    else:
        assert kind == "last70"
        m[n - 70:] = True
    return m


# (dim, n, c, B, list, id_offset): every value of every axis, every (units per lane, rows in flight); "five" / "one" / "last70"
# with a larger c are the lists shorter than c (padding)
ONE_LIST_CASES = [
    (16, 4099, 64, 4, "all", 0), (16, 1000, 1, 1, "one", 0), (16, 4099, 257, 3, "random", 0), (16, 1000, 20, 5, "five", 0),
    (48, 1000, 65, 3, "second", 0), (48, 4099, 20, 5, "last70", 0), (48, 4099, 256, 9, "random", 0), (48, 1000, 1024, 1, "all", 0),
    (512, 4099, 256, 9, "random", 0), (512, 1000, 257, 1, "five", 0), (512, 4099, 1024, 4, "all", 0), (512, 1000, 64, 5, "last70", 0),
    (528, 4099, 1, 1, "all", 0), (528, 1000, 257, 4, "second", 1000), (528, 1000, 20, 5, "five", 0),
    (768, 4099, 20, 1, "random", 0), (768, 4099, 1024, 4, "all", 0), (768, 4099, 64, 9, "second", 0), (768, 1000, 65, 3, "last70", 0),
    (768, 4099, 256, 5, "random", 7), (768, 1000, 20, 4, "one", 0), (768, 1000, 1024, 3, "last70", 0),
    (1040, 4099, 65, 1, "random", 3), (1040, 1000, 257, 5, "all", 0), (1280, 1000, 20, 4, "random", 0), (1536, 1000, 64, 1, "second", 0),
    (2064, 1000, 20, 5, "random", 0), (2064, 1000, 257, 1, "five", 0), (3104, 1000, 257, 1, "second", 0), (3104, 1000, 20, 4, "last70", 0),
    (4096, 1000, 64, 1, "random", 0), (4096, 1000, 1024, 3, "all", 0), (4096, 1000, 20, 4, "five", 0),
]


@pytest.mark.parametrize("dim,n,c,b,kind,id_offset", ONE_LIST_CASES)
def test_one_list_records_equal_the_model(dim, n, c, b, kind, id_offset):
    S = setup(dim, n)
    mask = list_mask(kind, n, dim + c)
    Q_dev, qc, qs = queries(S, b, c + b, first=int(np.flatnonzero(mask)[0]))
    buf, n_a = filter_dev(mask, dim)
    got = one_list_dev(S, Q_dev, c, buf, n_a, id_offset)
    want = lm.candidates_filtered(S.rc, S.rsc, qc, qs, S.dewi, S.ent, c, mask, id_offset)
    assert_records_equal(got, want, f"{dim} x {n}, c {c}, B {b}, list {kind}")
    m = min(c, n_a)
    assert mask[got["id"][:, :m] - id_offset].all(), "a row outside the list"
    assert (got["id"][:, m:] == -1).all() and np.isneginf(got["sim"][:, m:]).all()
    if kind == "last70":
        assert (got["id"][:, :m] - id_offset == n - 1).any(axis=1).all() or c < 70
    if kind == "all":
        plain = candidates_dev(S.codes, S.scales, Q_dev, S.dewi_dev, S.ent_dev, c, id_offset)
        assert_records_equal(got, plain, "every row: the unfiltered call")


def test_list_splits_identical_rows_nan_rows_first():
    dim, n, c, b, id_offset = 768, 1000, 50, 3, 11
    S = setup(dim, n, "ties")                        # rows 100 .. 139 are copies of row 5; rows 7 and n - 1 NaN; row 300 zero
    mask = np.ones(n, bool)
    mask[100:140:2] = False                          # the list keeps every second copy
    mask[5] = False
    Q_dev, qc, qs = queries(S, b, 3, first=5)
    buf, n_a = filter_dev(mask, dim)
    got = one_list_dev(S, Q_dev, c, buf, n_a, id_offset)
    want = lm.candidates_filtered(S.rc, S.rsc, qc, qs, S.dewi, S.ent, c, mask, id_offset)
    assert_records_equal(got, want, "ties")
    first = got["id"][0] - id_offset
    assert np.isnan(got["sim"][0, :2]).all() and first[:2].tolist() == [7, n - 1]
    assert first[2:22].tolist() == list(range(101, 140, 2))
    mask[[7, n - 1]] = False                         # without the NaN rows
    buf, n_a = filter_dev(mask, dim)
    got = one_list_dev(S, Q_dev, c, buf, n_a, id_offset)
    assert (got["id"][0, :20] - id_offset).tolist() == list(range(101, 140, 2)) and not np.isnan(got["sim"]).any()


@pytest.mark.parametrize("dim,c", [(48, 20), (768, 257), (2064, 64)])
def test_disallowed_rows_never_appear(dim, c):
    """Every disallowed row is overwritten with the query's own codes at a large scale: each would be the best row by far."""
    import torch
    n, b = 1000, 4
    S = setup(dim, n)
    mask = np.random.RandomState(dim).rand(n) < 0.4
    Q_dev, qc, qs = queries(S, b, 5, first=int(np.flatnonzero(mask)[0]))
    codes, scales = S.codes.clone(), S.scales.clone()
    out_rows = torch.from_numpy(np.flatnonzero(~mask)).cuda()
    codes[out_rows] = torch.from_numpy(qc[0]).cuda()
    scales[out_rows] = 1.0e6
    buf, n_a = filter_dev(mask, dim)
    got = one_list_dev(S, Q_dev, c, buf, n_a, codes=codes, scales=scales)
    want = lm.candidates_filtered(codes.cpu().numpy(), scales.cpu().numpy(), qc, qs, S.dewi, S.ent, c, mask)
    assert_records_equal(got, want, "planted rows")
    assert mask[got["id"]].all()
    # the planted rows do win where they are allowed
    buf_all, _ = filter_dev(np.ones(n, bool), dim)
    assert not mask[one_list_dev(S, Q_dev, c, buf_all, n, codes=codes, scales=scales)["id"][0, 0]]


def query_masks(b, n, c, seed):
    """Random lists of 30 .. 60 % of the rows; one equal to all rows, two disjoint ones, one of exactly c rows."""
    rs = np.random.RandomState(seed)
    masks = np.stack([rs.rand(n) < p for p in rs.uniform(0.3, 0.6, b)])
    exact = np.zeros(n, bool)
    exact[rs.choice(n, c, replace=False)] = True
    if b >= 5:
        masks[0] = True
        masks[1], masks[2] = np.arange(n) % 2 == 0, np.arange(n) % 2 == 1
        masks[3] = exact
    else:
        masks[0], masks[b - 1] = exact, True
    assert (masks.sum(axis=1) >= c).all()
    return masks


@pytest.mark.parametrize("dim,b,c", [(768, 2, 20), (768, 5, 257), (768, 8, 1024), (768, 37, 20), (48, 37, 257), (48, 5, 1024),
                                     (48, 8, 20), (512, 2, 257), (2064, 5, 20), (4096, 8, 257), (1040, 37, 1024)])
def test_per_query_lists_equal_the_model_and_the_one_list_call(dim, b, c):
    n = 4099
    S = setup(dim, n)
    masks = query_masks(b, n, c, dim + b + c)
    Q_dev, qc, qs = queries(S, b, b + c, first=int(np.flatnonzero(masks[0])[0]))
    buf, n_u, counts = query_filter_dev(masks, dim)
    got = per_query_dev(S, Q_dev, c, buf, n_u, counts, id_offset=2)
    want = lm.candidates_filtered(S.rc, S.rsc, qc, qs, S.dewi, S.ent, c, masks, 2)
    assert_records_equal(got, want, f"{dim}, B {b}, c {c}")
    for j in range(b):
        assert masks[j][got["id"][j] - 2].all(), j
    for j in range(b):
        fbuf, n_a = filter_dev(masks[j], dim)
        single = one_list_dev(S, Q_dev[j:j + 1], c, fbuf, n_a, id_offset=2)
        assert_records_equal(got[j:j + 1], single, f"query {j} on its own list")


def test_per_query_call_refuses_a_short_list_before_any_device_work():
    from dewi import _native as nat
    S = setup(48, 1000)
    masks = np.zeros((2, 1000), bool)
    masks[0, :100], masks[1, :10] = True, True
    Q_dev, _, _ = queries(S, 2, 1)
    buf, n_u, counts = query_filter_dev(masks, 48)
    with pytest.raises(ValueError, match="query 1: 10 allowed rows < the batch's cut 20"):
        per_query_dev(S, Q_dev, 20, buf, n_u, counts)
    assert "search it on its own filter" in nat.last_error()


# ------------------------------------------------------------------------------------------------------------ probe buffers
@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("c", [20, 257])
def test_probe_buffers_from_an_assign_array(dim, c):
    """``dewi_ivf_lists_build`` + ``dewi_ivf_probe_prepare`` (16 cells, nprobe 3, 11 queries: groups of 8 + 3): the list of a
    group is not ascending across cell segments.  Rows 5, 700 and 1500 are one vector in three cells: the lower row wins."""
    import torch
    from dewi import _native as nat
    lib = _lib()
    n, cells, nprobe, b, group = 4099, 16, 3, 11, 8
    key = ("probe", dim)
    if key not in _cache:
        S = Setup(dim, n)
        x = S.x.copy()
        x[700], x[1500] = x[5], x[5]
        S.x = x
        S.E_dev = torch.from_numpy(x).cuda()
        S.codes, S.scales = quantize_dev(S.E_dev)
        S.rc, S.rsc = S.codes.cpu().numpy(), S.scales.cpu().numpy()
        _cache[key] = S
    S = _cache[key]
    rs = np.random.RandomState(dim)
    assign = rs.randint(0, cells, n).astype(np.int32)
    assign[5], assign[700], assign[1500] = 9, 2, 5            # the lowest row sits in the highest cell: last in the list
    probe = np.stack([rs.choice(cells, nprobe, replace=False) for _ in range(b)]).astype(np.int64)
    probe[0], probe[9] = [9, 2, 5], [5, 9, 2]
    Q_dev, qc, qs = queries(S, b, 3, first=5)
    q = Q_dev.cpu().numpy()
    q[9] = S.x[5]
    Q_dev = torch.from_numpy(q).cuda()
    qc, qs, _ = prepare_dev(Q_dev)
    a_dev, p_dev = torch.from_numpy(assign).cuda(), torch.from_numpy(probe).cuda()
    need = int(lib.dewi_ivf_lists_bytes(n, dim, 0, cells))
    lists = torch.empty(need, dtype=torch.uint8, device="cuda")
    nat.check(lib.dewi_ivf_lists_build(0, n, dim, cells, nat.ptr(a_dev), nat.ptr(lists), need, nat.stream_ptr()))
    need = int(lib.dewi_ivf_probe_bytes(n, dim, 0, b, group))
    stride = int(lib.dewi_ivf_probe_group_bytes(n, dim, 0, group))
    pbuf = torch.empty(need, dtype=torch.uint8, device="cuda")
    n_union, n_allowed = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * b)()
    nat.check(lib.dewi_ivf_probe_prepare(0, n, dim, nat.ptr(lists), cells, nat.ptr(p_dev), b, nprobe, group, nat.ptr(pbuf), need,
                                         n_union, n_allowed, nat.stream_ptr()))
    masks = np.stack([np.isin(assign, probe[j]) for j in range(b)])
    assert list(n_allowed) == masks.sum(axis=1).tolist() and min(n_allowed) >= c
    want = lm.candidates_filtered(S.rc, S.rsc, qc, qs, S.dewi, S.ent, c, masks)
    for g, q0 in enumerate((0, 8)):
        nq = min(group, b - q0)
        rows = pbuf[g * stride:].view(torch.int32)[16:16 + n_union[g]].cpu().numpy()
        assert (np.diff(rows) < 0).any(), "the probe list is expected not to be ascending"
        got = per_query_dev(S, Q_dev[q0:q0 + nq], c, pbuf[g * stride:], n_union[g], list(n_allowed[q0:q0 + nq]))
        assert_records_equal(got, want[q0:q0 + nq], f"group {g}")
        if g == 0:
            assert got["id"][0, :3].tolist() == [5, 700, 1500] and len(set(got["sim"][0, :3].tolist())) == 1
        else:
            assert got["id"][1, :3].tolist() == [5, 700, 1500]


# ------------------------------------------------------------------------------------------------------------ workspace contract
@pytest.mark.parametrize("dim", [48, 768])
@pytest.mark.parametrize("c", [20, 300])
@pytest.mark.parametrize("entry", ["one", "per_query"])
def test_workspace_contract(dim, c, entry):
    """Results do not depend on what the workspace held (list form: slots no row reached; dense form: the slots of queries
    whose bit is clear); nothing outside the workspace or the records is written."""
    import torch
    n, b = 2100, 5
    S = setup(dim, n)
    rs = np.random.RandomState(c)
    Q_dev, _, _ = queries(S, b, c)
    if entry == "one":
        mask = rs.rand(n) < 0.35
        buf, n_scan = filter_dev(mask, dim)
        run = lambda ws, out: one_list_dev(S, Q_dev, c, buf, n_scan, 3, ws=ws, out=out)
    else:
        masks = np.stack([rs.rand(n) < p for p in (0.2, 0.5, 0.3, 0.9, 0.25)])
        buf, n_scan, counts = query_filter_dev(masks, dim)
        run = lambda ws, out: per_query_dev(S, Q_dev, c, buf, n_scan, counts, 3, ws=ws, out=out)
    need = int(_lib().dewi_knn_i8_filtered_workspace_bytes(n_scan, dim, b, c))
    base = None
    for i, pattern in enumerate(wsguard.PATTERNS):
        ws = wsguard.GuardedBuffer(need, "cuda", pattern, label=f"workspace ({entry}, {pattern})", seed=i)
        out = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="records")
        got = run(ws.view, out.mid)
        out.check()
        ws.check()
        if base is None:
            base = got
        assert same_bits(got, base), f"pattern {pattern}"

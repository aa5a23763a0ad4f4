"""Group quotas of the subset selection, the host side (no GPU): the four new symbols in header / ``EXPORTED_SYMBOLS`` / the
library's exports, every argument error of ``dewi_select_groups_begin`` / ``dewi_select_run_grouped`` /
``dewi_select_run_blocked_grouped`` (all raised before the first device call, so dummy host pointers do), the workspace size,
the Python surface, the dense-label helper and the ``seeds_count`` arithmetic."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NEW = {"dewi_select_grouped_workspace_bytes", "dewi_select_groups_begin", "dewi_select_run_grouped",
       "dewi_select_run_blocked_grouped"}
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -5

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer
INF = float("inf")
NAN = float("nan")
BIG = 1 << 40                                          # a workspace size no check refuses


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_header_symbol_list_and_exports_agree(lib):
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    declared = set(re.findall(r"\b(dewi_[a-z0-9_]+)\s*\(", header))
    assert NEW <= declared
    assert declared == set(nat.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("dewi_")}
    assert exported == declared, exported ^ declared
    assert lib.dewi_abi_version() == 6 == nat.ABI_VERSION


def need(n, n_groups):
    """the blocked layout (state, lists, unsafe, picks, ctl), then the records, the fill list and the counts,
    each region on a 256-byte boundary."""
    state = 2 * 256 * 8 + 256 + 9 * ((n + 63) // 64 * 64)
    blocked = (state + 255) // 256 * 256 + 256 * 17 * 8 + 256 * 4 + 64 * 8 + 256
    return (blocked + 255) // 256 * 256 + 256 + 256 + (4 * n_groups + 255) // 256 * 256


NEED = need(100, 7)


def begin(n=100, d=8, elem=0, groups=7, ws=P, nbytes=BIG):
    return lambda lib: lib.dewi_select_groups_begin(n, d, elem, groups, ws, nbytes, None)


def run(E=P, elem=0, n=100, d=8, rel=P, budget=5, lam=0.5, max_sim=INF, rows=P, gain=P, cnt=P, pen=None, owner=None, ws=P,
        nbytes=BIG, labels=P, groups=7, quota=None, per_group=1, counts=None):
    return lambda lib: lib.dewi_select_run_grouped(E, elem, n, d, rel, budget, lam, max_sim, 0, rows, gain, cnt, pen, owner, ws,
                                                   nbytes, None, labels, groups, quota, per_group, counts)


def blk(E=P, elem=0, n=100, d=8, rel=P, budget=5, lam=0.5, max_sim=INF, rows=P, gain=P, cnt=P, ws=P, nbytes=BIG, block=4,
        n_rounds=3, stats=None, labels=P, groups=7, quota=None, per_group=1, counts=None):
    return lambda lib: lib.dewi_select_run_blocked_grouped(E, elem, n, d, rel, budget, lam, max_sim, 0, rows, gain, cnt, None, None,
                                                           ws, nbytes, None, block, n_rounds, stats, labels, groups, quota,
                                                           per_group, counts)


SHORT = f"workspace {NEED - 1} B < required {NEED} B"
CASES = [
    ("begin: rows", begin(n=0), INVALID, "bad shape 0 x 8"),
    ("begin: rows 2^31", begin(n=1 << 31), UNSUPPORTED, "n_rows 2147483648: a subset selection takes fewer than 2^31 rows"),
    ("begin: elem_type", begin(elem=3), INVALID, "unknown elem_type 3"),
    ("begin: no groups", begin(groups=0), INVALID, "n_groups 0 outside [1, 2^31-1]"),
    ("begin: groups 2^31", begin(groups=1 << 31), INVALID, "n_groups 2147483648 outside [1, 2^31-1]"),
    ("begin: null workspace", begin(ws=None), WORKSPACE, f"workspace {BIG} B < required {NEED} B"),
    ("begin: short workspace", begin(nbytes=NEED - 1), WORKSPACE, SHORT),
    ("begin: the plain size is short", begin(nbytes=2 * 256 * 8 + 256 + 9 * 128), WORKSPACE,
     f"workspace {2 * 256 * 8 + 256 + 9 * 128} B < required {NEED} B"),
    ("begin: order: the shape before the groups", begin(n=0, groups=0), INVALID, "bad shape 0 x 8"),
    ("begin: order: the groups before the workspace", begin(groups=-2, ws=None), INVALID, "n_groups -2 outside [1, 2^31-1]"),
]
for name, call in (("run", run), ("blocked", blk)):
    CASES += [
        (f"{name}: null corpus", call(E=None), INVALID, "null pointer"),
        (f"{name}: null relevance", call(rel=None), INVALID, "null pointer"),
        (f"{name}: null rows", call(rows=None), INVALID, "null pointer"),
        (f"{name}: null gain", call(gain=None), INVALID, "null pointer"),
        (f"{name}: null counter", call(cnt=None), INVALID, "null pointer"),
        (f"{name}: null labels", call(labels=None), INVALID, "null pointer"),
        (f"{name}: no groups", call(groups=0), INVALID, "n_groups 0 outside [1, 2^31-1]"),
        (f"{name}: groups 2^31", call(groups=1 << 31), INVALID, "n_groups 2147483648 outside [1, 2^31-1]"),
        (f"{name}: per_group 0", call(per_group=0), INVALID, "per_group must be at least 1 (got 0)"),
        (f"{name}: per_group < 0", call(per_group=-4), INVALID, "per_group must be at least 1 (got -4)"),
        (f"{name}: per_group is not read beside a quota array", call(per_group=0, quota=P, budget=0), OK, None),
        (f"{name}: lambda above", call(lam=1.5), INVALID, "mmr_lambda 1.5 outside [0, 1]"),
        (f"{name}: lambda NaN", call(lam=NAN), INVALID, "mmr_lambda nan outside [0, 1]"),
        (f"{name}: max_sim NaN", call(max_sim=NAN), INVALID, "max_sim is NaN"),
        (f"{name}: rows", call(n=-5), INVALID, "bad shape -5 x 8"),
        (f"{name}: dim", call(d=0), INVALID, "bad shape 100 x 0"),
        (f"{name}: rows 2^31", call(n=(1 << 31) + 5), UNSUPPORTED,
         "n_rows 2147483653: a subset selection takes fewer than 2^31 rows"),
        (f"{name}: elem_type", call(elem=2), INVALID, "unknown elem_type 2"),
        (f"{name}: null workspace", call(ws=None), WORKSPACE, f"workspace {BIG} B < required {NEED} B"),
        (f"{name}: short workspace", call(nbytes=NEED - 1), WORKSPACE, SHORT),
        (f"{name}: budget 0 writes nothing", call(budget=0), OK, None),
        (f"{name}: budget < 0", call(budget=-7), OK, None),
        (f"{name}: order: the pointers before the groups", call(E=None, groups=0), INVALID, "null pointer"),
        (f"{name}: order: the labels before the groups", call(labels=None, groups=0), INVALID, "null pointer"),
        (f"{name}: order: the groups before per_group", call(groups=0, per_group=0), INVALID, "n_groups 0 outside [1, 2^31-1]"),
        (f"{name}: order: per_group before lambda", call(per_group=0, lam=2.0), INVALID, "per_group must be at least 1 (got 0)"),
        (f"{name}: order: lambda before the shape", call(lam=2.0, n=0), INVALID, "mmr_lambda 2 outside [0, 1]"),
        (f"{name}: order: the workspace before budget <= 0", call(budget=0, nbytes=8), WORKSPACE, f"workspace 8 B < required {NEED} B"),
    ]
CASES += [
    ("blocked: n_rounds", blk(n_rounds=-1), INVALID, "n_rounds must not be negative (got -1)"),
    ("blocked: block 0", blk(block=0), INVALID, "block 0 outside [1, 64] (dewi_select_block_max of dim 8)"),
    ("blocked: block 65", blk(block=65), INVALID, "block 65 outside [1, 64] (dewi_select_block_max of dim 8)"),
    ("blocked: order: n_rounds before the shape", blk(n_rounds=-1, n=0), INVALID, "n_rounds must not be negative (got -1)"),
    ("blocked: order: the shape before the block", blk(block=0, n=0), INVALID, "bad shape 0 x 8"),
    ("blocked: order: the block before the workspace", blk(block=0, nbytes=8), INVALID,
     "block 0 outside [1, 64] (dewi_select_block_max of dim 8)"),
]


@pytest.mark.parametrize("name,call,code,message", CASES, ids=[c[0] for c in CASES])
def test_argument_error(lib, name, call, code, message):
    from dewi import _native as nat
    rc = call(lib)
    got = nat.last_error()
    print(f"{name}: rc {rc}, {got!r}")
    assert rc == code, (name, rc, got)
    if message is not None:
        assert got == message, name


def test_workspace_size(lib):
    """The blocked layout with the group regions behind it, at one offset whatever ``block`` — the grouped run calls take no
    ``block`` and either form continues the other —; 0 for what the calls refuse; the older size functions are unchanged."""
    size = lib.dewi_select_grouped_workspace_bytes
    assert size(100, 8, 0, 7, 0) == NEED
    for n, g in [(1, 1), (64, 64), (65, 3), (2053, 2053), (1_000_000, 1000), (1_000_000, 1_000_000)]:
        want = need(n, g)
        assert size(n, 768, 0, g, 0) == size(n, 768, 0, g, 32) == size(n, 50, 1, g, 1) == want and want % 256 == 0
        blocked = lib.dewi_select_blocked_workspace_bytes(n, 768, 0, 32)
        assert blocked == (4096 + 256 + 9 * ((n + 63) // 64 * 64) + 255) // 256 * 256 + 256 * 17 * 8 + 1024 + 512 + 256
        assert lib.dewi_select_workspace_bytes(n, 768, 0) == 4096 + 256 + 9 * ((n + 63) // 64 * 64)
        assert want - blocked <= 255 + 512 + 4 * g + 255          # the group regions: 512 bytes and one count per group
    for bad in [(0, 8, 0, 1, 0), (-1, 8, 0, 1, 0), (10, 0, 0, 1, 0), (10, 8, 2, 1, 0), (1 << 31, 8, 0, 1, 0), (10, 8, 0, 0, 0),
                (10, 8, 0, -1, 0), (10, 8, 0, 1 << 31, 0), (10, 8, 0, 1, -1), (10, 8, 0, 1, 65), (10, 8200, 0, 1, 4)]:
        assert size(*bad) == 0, bad
    assert size(10, 8200, 0, 1, 3) > 0 and size(10, 8, 0, (1 << 31) - 1, 0) > 4 * ((1 << 31) - 1)


def test_python_signatures():
    from dewi._engine import DeviceCorpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    want = ["self", "budget", "groups", "per_group", "quotas", "mmr_lambda", "max_sim", "relevance", "filter", "seeds",
            "seeds_count", "return_gain", "return_coverage", "picks_per_pass"]
    defaults = {"per_group": 1, "quotas": None, "mmr_lambda": 0.5, "max_sim": None, "relevance": None, "filter": None,
                "seeds": None, "seeds_count": True, "return_gain": False, "return_coverage": False, "picks_per_pass": 32}
    for cls in (ExactIndex, DewiIndex, IVFIndex):
        sig = inspect.signature(cls.select_subset_grouped)
        assert list(sig.parameters) == want, cls.__name__
        assert all(p.kind is p.KEYWORD_ONLY for name, p in sig.parameters.items() if name not in ("self", "budget"))
        assert sig.parameters["groups"].default is inspect.Parameter.empty
        assert {k: sig.parameters[k].default for k in defaults} == defaults
        plain = inspect.signature(cls.select_subset)
        assert list(plain.parameters) == ["self", "budget", "mmr_lambda", "max_sim", "relevance", "filter", "seeds", "return_gain",
                                          "return_coverage"], cls.__name__
    assert IVFIndex.select_subset_grouped is ExactIndex.select_subset_grouped
    sig = inspect.signature(DeviceCorpus.select_subset_device)
    assert list(sig.parameters)[:7] == ["self", "budget", "mmr_lambda", "max_sim", "relevance", "mask", "seeds"]
    new = ["group_labels", "n_groups", "per_group", "group_quota", "return_group_counts"]
    assert list(sig.parameters)[-5:] == new and all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in new)


def test_dense_labels():
    from dewi._engine import dense_group_labels, group_labels
    from dewi.backends import DuplicateGroups
    # sparse integers: dense in ascending order of the value, negatives ungrouped
    lab, codes = dense_group_labels(np.array([7, -1, 2_000_000_000, 7, -5, 0]), 6)
    assert lab.dtype == np.int32 and lab.tolist() == [1, -1, 2, 1, -1, 0] and codes == {0: 0, 7: 1, 2_000_000_000: 2}
    assert all(type(k) is int for k in codes)
    assert dense_group_labels([7, -1, 2_000_000_000, 7, -5, 0], 6)[0].tolist() == lab.tolist()
    # hashables: first appearance, None ungrouped
    lab, codes = dense_group_labels(["b.org", None, "a.com", "b.org", ("x", 1)], 5)
    assert lab.tolist() == [0, -1, 1, 0, 2] and codes == {"b.org": 0, "a.com": 1, ("x", 1): 2}
    assert dense_group_labels(np.array(["u", "v", "u"]), 3)[0].tolist() == [0, 1, 0]
    lab, codes = dense_group_labels([3, None, 3], 3)                 # integers beside None are hashables like any other
    assert lab.tolist() == [0, -1, 0] and codes == {3: 0}
    # a mapping doc_id -> value needs the index's rows; documents not named are ungrouped
    row_of = {"d0": 0, "d1": 1, "d2": 2, "d3": 3}
    lab, codes = dense_group_labels({"d3": "s", "d0": "t", "d1": None}, 4, row_of)
    assert lab.tolist() == [0, -1, -1, 1] and codes == {"t": 0, "s": 1}          # numbered in row order
    with pytest.raises(KeyError):
        dense_group_labels({"nobody": 1}, 4, row_of)
    with pytest.raises(ValueError):
        dense_group_labels({"d0": 1}, 4)
    # DuplicateGroups: its labels, whatever their values
    labels = np.array([4, 4, 9, 2, 9], np.int64)
    dup = DuplicateGroups(labels, np.ones(5, np.int64), labels.copy(), 3)
    lab, codes = dense_group_labels(dup, 5)
    assert lab.tolist() == [1, 1, 2, 0, 2] and codes == {2: 0, 4: 1, 9: 2}
    # no row grouped; the errors of group_labels; group_labels itself is what it was
    lab, codes = dense_group_labels([None, None], 2)
    assert lab.tolist() == [-1, -1] and codes == {}
    assert dense_group_labels(np.array([-1, -7]), 2)[0].tolist() == [-1, -1]
    for bad in ([1, 2, 3], np.zeros((2, 2), np.int64), np.array([0, 1 << 31])):
        with pytest.raises(ValueError):
            dense_group_labels(bad, 2)
    lab, n_groups = group_labels(np.array([7, -1, 7, 9, -1]), 5)
    assert lab.tolist() == [7, -1, 7, 9, -1] and n_groups == 4
    assert list(inspect.signature(group_labels).parameters) == ["groups", "n_rows", "row_of"]


def test_quotas_and_seeds_count_arithmetic():
    from dewi._engine import grouped_quotas
    codes = {"a": 0, "b": 1, "c": 2}
    assert grouped_quotas(codes, 3) is None                                   # per_group serves every group
    assert grouped_quotas(codes, 3, {"b": 7, "c": 0}).tolist() == [3, 7, 0]
    q = grouped_quotas(codes, 2, None, seed_labels=[0, 0, 0, 2, -1])           # three seeds in a, one in c, one ungrouped
    assert q.dtype == np.int32 and q.tolist() == [-1, 2, 1]
    assert grouped_quotas(codes, 2, {"a": 5}, seed_labels=[0, 1]).tolist() == [4, 1, 2]
    with pytest.raises(KeyError):
        grouped_quotas(codes, 2, {"d": 1})
    for bad in (0, -1):
        with pytest.raises(ValueError):
            grouped_quotas(codes, bad)


def test_l2_and_per_group_are_refused_before_anything_is_built():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    from dewi.types import Payload
    q = np.ones(4, np.float32)
    for idx in (ExactIndex(dim=4, space="l2"), IVFIndex(dim=4, space="l2"), DewiIndex(dim=4, space="l2")):
        idx.add("a", q, Payload())
        with pytest.raises(NotImplementedError, match="l2"):
            idx.select_subset_grouped(1, groups=[0])
    idx = ExactIndex(dim=4)
    idx.add("a", q, Payload())
    for bad in (0, -2):
        with pytest.raises(ValueError, match="per_group"):
            idx.select_subset_grouped(1, groups=[0], per_group=bad)

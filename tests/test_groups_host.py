"""Host side of the near-duplicate groups (no GPU): the five additive exports (still exactly the header, ABI 6), the argument
checks the entry points make before any device work, the Python surface, the answers that need no build, the shape of
``clusters``, and the NumPy model's own sanity on hand-written graphs."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import groups_model as gm

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"
NEW_EXPORTS = {"dewi_groups_workspace_bytes", "dewi_groups_begin", "dewi_groups_union_lists", "dewi_groups_union_pairs",
               "dewi_groups_finish"}


def _header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(dewi_\w+)\s*\(", src))


def _lib():
    from dewi import _native as nat
    return nat, nat.load_library(require_gpu=False)


def _dummy():
    """A 16-byte aligned host address: enough for an entry point that must return before it touches anything."""
    buf = ctypes.create_string_buffer(256)
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def test_groups_exports_equal_the_header():
    nat, lib = _lib()
    declared = _header_functions()
    assert NEW_EXPORTS <= declared
    assert NEW_EXPORTS <= set(nat.EXPORTED_SYMBOLS)
    assert set(nat.EXPORTED_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("dewi_")}
    assert exported == declared
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6
    text = HEADER.read_text()
    assert "#define DEWI_ABI_VERSION 6" in text
    assert "#define DEWI_GROUPS_KEEP_FIRST 0" in text and "#define DEWI_GROUPS_KEEP_MAX_KEY 1" in text
    assert nat.KEEP_CODES == {"first": 0, "dewi": 1}


def test_groups_workspace_bytes_needs_no_device():
    _, lib = _lib()
    ws = lib.dewi_groups_workspace_bytes
    for n in (0, -1, 1 << 31, 1 << 40):
        assert ws(n) == 0, n
    # parents (4 B) + member counts (4 B) + representative keys (8 B) per row, plus a small header: O(N), not O(pairs)
    for n in (1, 4097, 10007, 1 << 20, (1 << 31) - 1):
        assert 16 * n <= ws(n) <= 16 * n + 256, n
        assert ws(n) % 8 == 0


def test_groups_entry_points_check_their_arguments_before_any_device_work():
    nat, lib = _lib()
    keep, p = _dummy()
    big = 1 << 40
    too_many = (1 << 31)

    def begin(n=4097, ws=p, ws_bytes=big):
        return lib.dewi_groups_begin(n, ws, ws_bytes, None)

    def lists(n=4097, lims=p, rows=p, nq=257, t=1000, first=300, ws=p, ws_bytes=big):
        return lib.dewi_groups_union_lists(n, lims, rows, nq, t, first, ws, ws_bytes, None)

    def pairs(n=4097, a=p, b=p, m=1000, ws=p, ws_bytes=big):
        return lib.dewi_groups_union_pairs(n, a, b, m, ws, ws_bytes, None)

    n_groups, bad = ctypes.c_int64(-7), ctypes.c_int64(-7)

    def finish(n=4097, keep_rule=0, key=p, off=0, labels=p, sizes=p, reps=p, ng=ctypes.byref(n_groups), nb=ctypes.byref(bad), ws=p,
               ws_bytes=big):
        return lib.dewi_groups_finish(n, keep_rule, key, off, labels, sizes, reps, ng, nb, ws, ws_bytes, None)

    for fn in (begin, lists, pairs, finish):
        for kw in ({"n": 0}, {"n": -5}, {"n": too_many}, {"ws": p + 8}):
            assert fn(**kw) == nat.ERR_INVALID_ARG, (fn.__name__, kw)
        assert fn(ws=None) == nat.ERR_WORKSPACE, fn.__name__
        assert fn(ws_bytes=8) == nat.ERR_WORKSPACE, fn.__name__
        assert fn(ws_bytes=lib.dewi_groups_workspace_bytes(4097) - 1) == nat.ERR_WORKSPACE, fn.__name__
    for kw in ({"lims": None}, {"rows": None}, {"nq": 0}, {"nq": -1}, {"nq": 2049}, {"t": -1}, {"first": -1}, {"first": 4097 - 256},
               {"first": 4097}):
        assert lists(**kw) == nat.ERR_INVALID_ARG, kw
    for kw in ({"a": None}, {"b": None}, {"m": -1}):
        assert pairs(**kw) == nat.ERR_INVALID_ARG, kw
    for kw in ({"keep_rule": 2}, {"keep_rule": -1}, {"keep_rule": 1, "key": None}, {"labels": None}, {"sizes": None}, {"reps": None},
               {"ng": None}, {"nb": None}):
        assert finish(**kw) == nat.ERR_INVALID_ARG, kw
    assert n_groups.value == -7 and bad.value == -7                     # nothing was written
    # a count of zero is fine and launches nothing (no device is needed to say so)
    assert lists(t=0) == nat.OK and lists(t=0, rows=None) == nat.OK
    assert pairs(m=0) == nat.OK and pairs(m=0, a=None, b=None) == nat.OK
    with pytest.raises(ValueError):
        nat.check(begin(n=0))
    with pytest.raises(nat.NativeLibraryError):
        nat.check(begin(ws=None))
    del keep


def test_python_surface_of_the_groups():
    from dewi._engine import DeviceCorpus
    from dewi.backends import DuplicateGroups, ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    params = inspect.signature(DeviceCorpus.duplicate_groups_device).parameters
    assert list(params) == ["self", "threshold", "chunk", "use_shadow", "keep"]
    assert params["chunk"].default == 2048 and params["use_shadow"].default is True and params["keep"].default == "first"
    assert "max_pairs" not in params
    params = inspect.signature(DeviceCorpus.groups_from_pairs_device).parameters
    assert list(params) == ["self", "a", "b", "n_rows", "keep"]
    assert params["n_rows"].default is None and params["keep"].default == "first"
    for cls in (ExactIndex, DewiIndex):
        params = inspect.signature(cls.duplicate_groups).parameters
        assert list(params) == ["self", "threshold", "keep", "doc_ids"]
        assert params["keep"].default == "dewi" and params["doc_ids"].default is False
        params = inspect.signature(cls.dedup_filter).parameters
        assert list(params) == ["self", "threshold", "keep"] and params["keep"].default == "dewi"
    assert IVFIndex.duplicate_groups is ExactIndex.duplicate_groups and IVFIndex.dedup_filter is ExactIndex.dedup_filter
    assert [f.name for f in __import__("dataclasses").fields(DuplicateGroups)] == ["labels", "sizes", "representatives", "n_groups",
                                                                                   "clusters"]
    # the self-join keeps its signature
    assert list(inspect.signature(DeviceCorpus.near_duplicates_device).parameters) == ["self", "threshold", "chunk", "max_pairs",
                                                                                       "use_shadow"]


def test_duplicate_groups_of_an_empty_index_and_of_one_row_need_no_build():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.types import Payload
    for n in (0, 1):
        for make in (lambda: ExactIndex(8), lambda: DewiIndex(8)):
            for keep in ("dewi", "first"):
                idx = make()
                if n:
                    idx.add("d0", np.ones(8, np.float32), Payload())
                g = idx.duplicate_groups(0.5, keep=keep)
                for arr in (g.labels, g.sizes, g.representatives):
                    assert arr.dtype == np.int64 and arr.shape == (n,)
                assert g.n_groups == n and g.clusters is None
                if n:
                    assert g.labels[0] == 0 and g.sizes[0] == 1 and g.representatives[0] == 0
                g = idx.duplicate_groups(0.5, keep=keep, doc_ids=True)
                assert g.clusters == ([["d0"]] if n else [])
                backend = idx if isinstance(idx, ExactIndex) else idx._backend
                assert backend._corpus is None                          # nothing was built for it
    with pytest.raises(ValueError, match="keep"):
        ExactIndex(8).duplicate_groups(0.5, keep="last")


def test_clusters_are_ordered_by_label_then_row_and_include_singletons():
    from dewi.backends import clusters_from_labels
    ids = [f"d{i}" for i in range(8)]
    labels = np.array([0, 1, 0, 3, 1, 5, 0, 3], dtype=np.int64)
    clusters = clusters_from_labels(labels, ids)
    assert clusters == [["d0", "d2", "d6"], ["d1", "d4"], ["d3", "d7"], ["d5"]]
    assert sorted(x for c in clusters for x in c) == sorted(ids)          # a partition of all ids
    assert clusters_from_labels(np.arange(3), ids[:3]) == [["d0"], ["d1"], ["d2"]]
    assert clusters_from_labels(np.zeros(0, np.int64), []) == []


def test_the_model_on_hand_written_graphs():
    # two triangles that share no row, one bridge added later, singletons, a self-loop and a repeated edge
    a = [5, 6, 7, 1, 2, 9, 9, 2]
    b = [6, 7, 5, 2, 3, 9, 9, 1]
    labels, sizes, reps, n_groups = gm.groups(10, a, b)
    assert labels.tolist() == [0, 1, 1, 1, 4, 5, 5, 5, 8, 9]
    assert sizes.tolist() == [1, 3, 3, 3, 1, 3, 3, 3, 1, 1]
    assert reps.tolist() == labels.tolist() and n_groups == 6
    labels, sizes, _, n_groups = gm.groups(10, a + [3], b + [7])
    assert labels.tolist() == [0, 1, 1, 1, 4, 1, 1, 1, 8, 9] and sizes[1] == 6 and n_groups == 5
    # the order of the edges and of their endpoints does not matter
    r = np.random.RandomState(0)
    ea, eb = r.randint(0, 200, 150), r.randint(0, 200, 150)
    want = gm.groups(200, ea, eb)
    for seed in (1, 2):
        p = np.random.RandomState(seed).permutation(150)
        flip = np.random.RandomState(seed).rand(150) < 0.5
        got = gm.groups(200, np.where(flip, eb, ea)[p], np.where(flip, ea, eb)[p])
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3]
    for lab in np.unique(want[0]).tolist():                                # a label is its group's smallest row
        assert int(np.flatnonzero(want[0] == lab).min()) == lab
    # keep = "dewi": the largest key, ties to the lower row, NaN loses unless the group is all NaN, -0 == +0
    nan = np.float32("nan")
    key = np.array([1.0, 3.0, 3.0, nan, nan, nan, -np.inf, nan, -0.0, 0.0], np.float32)
    a, b = [0, 1, 4, 6, 8], [1, 2, 5, 7, 9]           # groups {0,1,2} {3} {4,5} {6,7} {8,9}
    labels, _, reps, _ = gm.groups(10, a, b, keep="dewi", key=key)
    assert labels.tolist() == [0, 0, 0, 3, 4, 4, 6, 6, 8, 8]
    assert reps.tolist() == [1, 1, 1, 3, 4, 4, 6, 6, 8, 8]


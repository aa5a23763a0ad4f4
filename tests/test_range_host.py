"""Host side of the range search (no GPU): the three additive exports (still exactly the header, ABI 6), the workspace size,
the argument checks the entry points make before any device work, and the Python checks that need no device."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"
NEW_EXPORTS = {"dewi_knn_range_workspace_bytes", "dewi_knn_range_count", "dewi_knn_range_collect"}


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


def test_range_exports_equal_the_header():
    nat, lib = _lib()
    declared = _header_functions()
    assert NEW_EXPORTS <= declared
    assert set(nat.EXPORTED_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("dewi_")}
    assert exported == declared
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6
    assert "#define DEWI_RANGE_MAX_QUERIES 32" in HEADER.read_text() and nat.RANGE_MAX_QUERIES == 32


def test_range_workspace_bytes_needs_no_device():
    _, lib = _lib()
    for n_scan, dim, elem in ((20000, 64, 0), (20000, 50, 0), (20011, 129, 0), (1 << 20, 768, 0), (20000, 96, 1), (1, 5, 0),
                              (257, 64, 0), ((1 << 32) - 1, 64, 0)):
        for nq in (1, 4, 31, 32):
            got = lib.dewi_knn_range_workspace_bytes(n_scan, dim, elem, nq)
            assert got >= 8 * nq * n_scan, (n_scan, dim, elem, nq)
            assert got <= 8 * nq * n_scan + 4 * nq * (n_scan // 1024 + 1) + 4 * nq * dim + 3 * 256, (n_scan, dim, elem, nq)
    for bad in ((0, 64, 0, 1), (-5, 64, 0, 1), (1 << 32, 64, 0, 1), (100, 0, 0, 1), (100, -1, 0, 1), (100, 64, 2, 1),
                (100, 64, -1, 1), (100, 64, 0, 0), (100, 64, 0, 33)):
        assert lib.dewi_knn_range_workspace_bytes(*bad) == 0, bad


def test_range_entry_points_check_their_arguments_before_any_device_work():
    nat, lib = _lib()
    keep, p = _dummy()
    big = 1 << 40

    def count(E=p, elem=0, n_rows=100, dim=64, filt=None, n_allowed=0, Q=p, nq=1, thr=p, space=0, counts=p, ws=p, ws_bytes=big):
        return lib.dewi_knn_range_count(E, elem, n_rows, dim, filt, n_allowed, Q, nq, thr, space, counts, ws, ws_bytes, None)

    for kw in ({"E": None}, {"Q": None}, {"thr": None}, {"counts": None}, {"nq": 0}, {"nq": 33}, {"space": 2}, {"space": -1},
               {"n_rows": 0}, {"dim": 0}, {"elem": 2}, {"filt": p, "n_allowed": 101}, {"filt": p, "n_allowed": -1},
               {"ws": p + 8}):
        assert count(**kw) == nat.ERR_INVALID_ARG, kw
    assert count(ws_bytes=8) == nat.ERR_WORKSPACE
    assert count(ws=None) == nat.ERR_WORKSPACE
    assert count(ws_bytes=lib.dewi_knn_range_workspace_bytes(100, 64, 0, 1) - 1) == nat.ERR_WORKSPACE
    assert count(filt=p, n_allowed=10, ws_bytes=8) == nat.ERR_WORKSPACE
    assert count(elem=1, filt=p, n_allowed=10) == nat.ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        nat.check(count(elem=1, filt=p, n_allowed=10))
    with pytest.raises(ValueError):
        nat.check(count(nq=33))

    def collect(ws=p, ws_bytes=big, n_scan=100, nq=1, thr=p, lims=p, cap=10, dewi=p, ent=p, rows=p, sims=p, scores=p):
        return lib.dewi_knn_range_collect(ws, ws_bytes, n_scan, nq, thr, lims, cap, dewi, ent, 0.5, 0.0, rows, sims, scores, None)

    for kw in ({"thr": None}, {"lims": None}, {"dewi": None}, {"ent": None}, {"rows": None}, {"sims": None}, {"scores": None},
               {"nq": 0}, {"nq": 33}, {"n_scan": -1}, {"n_scan": 1 << 32}, {"cap": -1}, {"ws": p + 8}):
        assert collect(**kw) == nat.ERR_INVALID_ARG, kw
    assert collect(ws_bytes=8) == nat.ERR_WORKSPACE and collect(ws=None) == nat.ERR_WORKSPACE
    assert collect(n_scan=0, ws=None) == nat.OK and collect(cap=0, ws=None) == nat.OK      # nothing to write
    del keep


def _tiny_index(cls=None, n=3, dim=8):
    from dewi.backends import ExactIndex
    from dewi.types import Payload
    idx = (cls or ExactIndex)(dim)
    idx.add_batch([f"d{i}" for i in range(n)], np.ones((n, dim), np.float32), [Payload() for _ in range(n)])
    return idx


def test_range_python_argument_checks_need_no_device():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    idx = _tiny_index()
    q = np.ones((2, 8), np.float32)
    with pytest.raises(ValueError, match="shape"):
        idx.range_search_batch(np.ones((2, 7), np.float32), 0.5)
    with pytest.raises(ValueError, match="shape"):
        idx.range_search_batch(np.ones(8, np.float32), 0.5)
    with pytest.raises(ValueError, match="shape"):
        idx.range_search(np.ones(9, np.float32), 0.5)
    for bad in ([0.5, 0.4, 0.3], np.zeros((2, 1), np.float32), []):
        with pytest.raises(ValueError, match="thresholds"):
            idx.range_search_batch(q, bad)
    with pytest.raises(NotImplementedError):
        idx.range_search_batch(q, 0.5, filter=np.ones((2, 3), dtype=bool))          # a bool [B, N] mask: per-query filters
    from dewi._engine import DeviceQueryFilters
    qf = DeviceQueryFilters(None, None, [3, 3], 3, 0, 3)
    with pytest.raises(NotImplementedError):
        idx.range_search_batch(q, 0.5, filter=qf)
    assert idx._corpus is None                                                      # none of this built anything
    face = DewiIndex(8)
    with pytest.raises(ValueError, match="shape"):
        face.range_search(np.ones((1, 8), np.float32), 0.5)
    with pytest.raises(ValueError, match="shape"):
        face.range_search_batch(np.ones(8, np.float32), 0.5)
    # signatures: the facade's defaults come from the constructor, IVFIndex inherits the exact methods and has no nprobe
    for name in ("range_search", "range_search_batch"):
        assert getattr(IVFIndex, name) is getattr(ExactIndex, name)
        assert "nprobe" not in inspect.signature(getattr(IVFIndex, name)).parameters
        params = inspect.signature(getattr(DewiIndex, name)).parameters
        assert params["eta"].default is None and params["entropy_pref"].default is None
    names = list(inspect.signature(ExactIndex.range_search).parameters)
    assert names == ["self", "query", "threshold", "eta", "entropy_pref", "filter", "max_results"]
    from dewi._engine import DeviceCorpus
    names = list(inspect.signature(DeviceCorpus.range_search_device).parameters)
    assert names == ["self", "q_dev", "thresholds", "eta", "entropy_pref", "filter", "max_results", "sort"]


def test_range_on_an_empty_index_is_empty():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    idx = ExactIndex(8)
    lims, rows, scores, sims = idx.range_search_batch(np.ones((3, 8), np.float32), 0.5)
    assert lims.tolist() == [0, 0, 0, 0] and lims.dtype == np.int64
    assert rows.shape == scores.shape == sims.shape == (0,)
    assert rows.dtype == np.int64 and scores.dtype == np.float32 and sims.dtype == np.float32
    assert idx.range_search(np.ones(8, np.float32), 0.5) == []
    face = DewiIndex(8)
    assert face.range_search(np.ones(8, np.float32), -1.0) == []
    assert face.range_search_batch(np.ones((2, 8), np.float32), [0.1, 0.2]) == [[], []]


def test_threshold_staging():
    from dewi._engine import check_thresholds
    assert check_thresholds(0.25, 3).tolist() == [0.25, 0.25, 0.25]
    assert check_thresholds([0.5], 2).tolist() == [0.5, 0.5]
    got = check_thresholds(np.array([0.1, 0.2], np.float64), 2)
    assert got.dtype == np.float32 and got.flags.c_contiguous and got.tolist() == [np.float32(0.1), np.float32(0.2)]
    with pytest.raises(ValueError):
        check_thresholds([0.1, 0.2], 3)

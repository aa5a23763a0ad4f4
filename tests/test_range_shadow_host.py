"""Host side of the range search through the bf16 shadow and of the near-duplicate self-join (no GPU): the four additive
exports (still exactly the header, ABI 6), the shapes the workspace function refuses, the argument checks the entry points
make before any device work, and the Python surface."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"
NEW_EXPORTS = {"dewi_knn_range_shadow_supported", "dewi_knn_range_shadow_workspace_bytes", "dewi_knn_range_shadow_count",
               "dewi_knn_range_shadow_collect"}
COSINE, L2 = 0, 1


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


def test_range_shadow_exports_equal_the_header():
    nat, lib = _lib()
    declared = _header_functions()
    assert NEW_EXPORTS <= declared
    assert NEW_EXPORTS <= set(nat.EXPORTED_SYMBOLS)
    assert set(nat.EXPORTED_SYMBOLS) == declared
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("dewi_")}
    assert exported == declared
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6
    assert "#define DEWI_RANGE_SHADOW_MAX_QUERIES 2048" in HEADER.read_text() and nat.RANGE_SHADOW_MAX_QUERIES == 2048
    assert "#define DEWI_ABI_VERSION 6" in HEADER.read_text()


def test_the_header_states_the_planners_rule_for_the_shadow_search():
    text = HEADER.read_text()
    assert "dim % 8 == 0 from 136 to 1536" in text and "dim % 32 == 0 from 160" not in text


def test_range_shadow_supported_shapes_need_no_device():
    _, lib = _lib()
    for dim in (256, 384, 512, 640, 768):
        for n in (32, 40011, 1 << 20):
            assert lib.dewi_knn_range_shadow_supported(n, dim, COSINE) == 1, (n, dim)
        assert lib.dewi_knn_range_shadow_supported(40011, dim, L2) == 0
        assert lib.dewi_knn_range_shadow_supported(40011, dim, 7) == 0
    for dim in (128, 200, 260, 896, 1024, 0, -256):
        assert lib.dewi_knn_range_shadow_supported(40011, dim, COSINE) == 0, dim
    # a row floor, if any, may not exceed 32 768 rows
    assert lib.dewi_knn_range_shadow_supported(32768, 768, COSINE) == 1
    for n in (0, -1, 1 << 31):
        assert lib.dewi_knn_range_shadow_supported(n, 768, COSINE) == 0, n


def test_range_shadow_workspace_bytes_refuses_without_a_device():
    _, lib = _lib()
    ws = lib.dewi_knn_range_shadow_workspace_bytes
    for dim in (128, 200, 896):
        assert ws(40011, dim, COSINE, 300, 32) == 0, dim
    assert ws(40011, 768, L2, 300, 32) == 0
    for nq in (0, -1, 2049):
        assert ws(40011, 768, COSINE, nq, 32) == 0, nq
    for cap in (0, -4, 1 << 19, (1 << 31) - 1):     # 4 segments x 256 queries x 8 bytes x 2^19 records = 2^32: no device takes it
        assert ws(40011, 768, COSINE, 300, cap) == 0, cap
    assert ws(0, 768, COSINE, 300, 32) == 0


def test_range_shadow_entry_points_check_their_arguments_before_any_device_work():
    nat, lib = _lib()
    keep, p = _dummy()
    big = 1 << 40

    def count(E=p, Eb=p, n_rows=40011, dim=768, first=0, Q=p, nq=300, thr=p, cap=32, counts=p, ws=p, ws_bytes=big):
        return lib.dewi_knn_range_shadow_count(E, Eb, n_rows, dim, first, Q, nq, thr, cap, counts, ws, ws_bytes, None)

    for kw in ({"E": None}, {"Eb": None}, {"Q": None}, {"thr": None}, {"counts": None}, {"nq": 0}, {"nq": 2049}, {"n_rows": 0},
               {"dim": 0}, {"first": -1}, {"first": 40011}, {"cap": 0}, {"cap": -1}, {"cap": 1 << 19}, {"ws": p + 8}):
        assert count(**kw) == nat.ERR_INVALID_ARG, kw
    for kw in ({"dim": 128}, {"dim": 200}, {"dim": 896}, {"n_rows": 31}):
        assert count(**kw) == nat.ERR_UNSUPPORTED, kw
    assert count(ws=None) == nat.ERR_WORKSPACE and count(ws_bytes=8) == nat.ERR_WORKSPACE
    with pytest.raises(ValueError):
        nat.check(count(nq=2049))
    with pytest.raises(NotImplementedError):
        nat.check(count(dim=896))

    def collect(ws=p, ws_bytes=big, n_rows=40011, dim=768, first=0, nq=300, cap=32, lims=p, capacity=10, dewi=p, ent=p, rows=p,
                sims=p, scores=p):
        return lib.dewi_knn_range_shadow_collect(ws, ws_bytes, n_rows, dim, first, nq, cap, lims, capacity, dewi, ent, 0.5, 0.0,
                                                 rows, sims, scores, None)

    for kw in ({"lims": None}, {"dewi": None}, {"ent": None}, {"rows": None}, {"sims": None}, {"scores": None}, {"nq": 0},
               {"nq": 2049}, {"n_rows": 0}, {"dim": 0}, {"first": -1}, {"first": 40011}, {"cap": 0}, {"cap": 1 << 19},
               {"capacity": -1}, {"ws": p + 8}):
        assert collect(**kw) == nat.ERR_INVALID_ARG, kw
    for kw in ({"dim": 128}, {"dim": 896}):
        assert collect(**kw) == nat.ERR_UNSUPPORTED, kw
    assert collect(ws=None) == nat.ERR_WORKSPACE and collect(ws_bytes=8) == nat.ERR_WORKSPACE
    del keep


def test_python_surface_of_the_shadow_route_and_the_self_join():
    from dewi import _engine
    from dewi._engine import DeviceCorpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    # range_search_device keeps its parameter list (the shadow route is its default); the route switch is range_search_routed's
    names = list(inspect.signature(DeviceCorpus.range_search_device).parameters)
    params = inspect.signature(DeviceCorpus.range_search_routed).parameters
    assert list(params) == names + ["use_shadow"] and params["use_shadow"].default is True
    params = inspect.signature(DeviceCorpus.near_duplicates_device).parameters
    assert list(params) == ["self", "threshold", "chunk", "max_pairs", "use_shadow"]
    assert params["chunk"].default == 2048 and params["max_pairs"].default is None and params["use_shadow"].default is True
    assert list(inspect.signature(ExactIndex.near_duplicates).parameters) == ["self", "threshold", "max_pairs", "doc_ids"]
    assert list(inspect.signature(DewiIndex.near_duplicates).parameters) == ["self", "threshold", "max_pairs", "doc_ids"]
    assert IVFIndex.near_duplicates is ExactIndex.near_duplicates
    assert 1 <= _engine.RANGE_SHADOW_MIN_BATCH <= 2048


def test_near_duplicates_of_an_empty_index_and_of_one_row_are_empty():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.types import Payload
    for n in (0, 1):
        for idx in (ExactIndex(8), DewiIndex(8)):
            if n:
                idx.add("d0", np.ones(8, np.float32), Payload())
            a, b, sims = idx.near_duplicates(0.5)
            assert a.shape == b.shape == sims.shape == (0,)
            assert a.dtype == np.int64 and b.dtype == np.int64 and sims.dtype == np.float32
            ia, ib, sims = idx.near_duplicates(0.5, doc_ids=True)
            assert ia == [] and ib == [] and sims.shape == (0,)
    assert ExactIndex(8)._corpus is None            # nothing was built for it

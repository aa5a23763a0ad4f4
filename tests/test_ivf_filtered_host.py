"""Host side of the IVF probe under a user filter (library loaded, no GPU): the three additive exports (declared, bound and
documented; still ABI 6), the two size functions, the argument errors of ``dewi_ivf_probe_prepare_filtered`` — all raised before
any device work — and the ``ValueError``s of ``IVFIndex.search_probe_filtered*`` that need no device."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"
NEW_EXPORTS = ("dewi_ivf_probe_filtered_group_bytes", "dewi_ivf_probe_filtered_bytes", "dewi_ivf_probe_prepare_filtered")


def _lib():
    from dewi import _native as nat
    return nat, nat.load_library(require_gpu=False)


def test_exports_are_declared_bound_and_documented():
    nat, lib = _lib()
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for name in NEW_EXPORTS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert name in nat.EXPORTED_SYMBOLS
        assert re.search(rf"\b{name}\b", comments), f"{name} is not documented"
        assert getattr(lib, name).argtypes is not None
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6
    for word in ("allow_per_query", "out_n_allowed", "SYNCHRONISES"):
        assert word in comments


def test_size_functions_need_no_device():
    nat, lib = _lib()
    for n, dim in ((20000, 64), (20000, 50), (1 << 20, 768), (600, 129), (1, 64)):
        for group in (1, 8, 32):
            stride = lib.dewi_ivf_probe_filtered_group_bytes(n, dim, 0, group)
            assert stride > 0 and stride % 4 == 0
            assert stride >= lib.dewi_ivf_probe_group_bytes(n, dim, 0, group)
            for b in (1, group, group + 1, 4 * group):
                groups = (b + group - 1) // group
                got = lib.dewi_ivf_probe_filtered_bytes(n, dim, 0, b, group)
                assert got > 0 and got % 4 == 0
                assert got >= lib.dewi_ivf_probe_bytes(n, dim, 0, b, group), (n, dim, group, b)
                assert got >= groups * stride + 4 * (groups + b), (n, dim, group, b)
    for bad in ((0, 64, 0, 4, 8), (100, 0, 0, 4, 8), (100, 64, 2, 4, 8), (100, 64, 0, 0, 8), (100, 64, 0, 4, 0),
                (100, 64, 0, 4, 33), (100, 64, 0, 65536, 8), (1 << 33, 64, 0, 4, 8)):
        assert lib.dewi_ivf_probe_filtered_bytes(*bad) == 0, bad
    for bad in ((0, 64, 0, 8), (100, 0, 0, 8), (100, 64, 2, 8), (100, 64, 0, 0), (100, 64, 0, 33)):
        assert lib.dewi_ivf_probe_filtered_group_bytes(*bad) == 0, bad


def test_entry_point_refuses_bad_arguments_before_any_device_work():
    nat, lib = _lib()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    cnt = (ctypes.c_int64 * 4)()
    f = lib.dewi_ivf_probe_prepare_filtered
    big = 1 << 20
    assert f(1, 100, 64, p, 4, p, 2, 1, 8, p, 0, p, big, cnt, cnt, None) == nat.ERR_UNSUPPORTED        # bf16
    assert f(2, 100, 64, p, 4, p, 2, 1, 8, p, 0, p, big, cnt, cnt, None) != nat.OK                      # no such elem_type
    assert f(0, 100, 64, p, 4, p, 2, 5, 8, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG        # nprobe > cells
    assert f(0, 100, 64, p, 4, p, 2, 0, 8, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG
    assert f(0, 100, 64, p, 4, p, 2, 1, 33, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG       # group
    assert f(0, 100, 64, p, 4, p, 2, 1, 0, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG
    assert f(0, 100, 64, p, 0, p, 2, 1, 8, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG        # n_cells
    assert f(0, 100, 64, p, 101, p, 2, 1, 8, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG
    assert f(0, 100, 64, p, 4, p, 0, 1, 8, p, 0, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG        # n_queries
    assert f(0, 100, 64, p, 4, p, 2, 1, 8, p, 2, p, big, cnt, cnt, None) == nat.ERR_INVALID_ARG        # allow_per_query
    assert f(0, 100, 64, p, 4, p, 2, 1, 8, p, 0, p, 8, cnt, cnt, None) == nat.ERR_WORKSPACE            # a short buffer
    need = lib.dewi_ivf_probe_filtered_bytes(100, 64, 0, 2, 8)
    assert f(0, 100, 64, p, 4, p, 2, 1, 8, p, 1, p, need - 1, cnt, cnt, None) == nat.ERR_WORKSPACE
    # the unfiltered size is not enough
    assert f(0, 100, 64, p, 4, p, 2, 1, 8, p, 0, p, lib.dewi_ivf_probe_bytes(100, 64, 0, 2, 8), cnt, cnt, None) == nat.ERR_WORKSPACE
    for null in (3, 5, 9, 11, 13, 14):                                                                  # each pointer in turn
        args = [0, 100, 64, p, 4, p, 2, 1, 8, p, 0, p, big, cnt, cnt, None]
        args[null] = None
        assert f(*args) == nat.ERR_INVALID_ARG, null
    with pytest.raises(NotImplementedError):
        nat.check(f(1, 100, 64, p, 4, p, 2, 1, 8, p, 0, p, big, cnt, cnt, None))


def _index(**kwargs):
    from dewi.ivf import IVFIndex
    from dewi.types import Payload
    idx = IVFIndex(16, **kwargs)
    idx.add_batch(["a", "b"], np.ones((2, 16), np.float32), [Payload(), Payload()])
    return idx


def test_python_argument_errors_need_no_device():
    q1, qb, mask = np.ones(16, np.float32), np.ones((2, 16), np.float32), np.ones(2, bool)
    plain, codes = _index(), _index(int8_codes=True)
    calls = {
        "filter=None": lambda: plain.search_probe_filtered(q1, 1, filter=None),
        "filter=None, batch": lambda: plain.search_probe_filtered_batch(qb, 1, filter=None),
        "filter=None, device": lambda: plain.search_probe_filtered_device(qb, 1, filter=None),
        "approx without codes": lambda: plain.search_probe_filtered_batch(qb, 1, filter=mask, approx=True),
        "approx with a transform": lambda: codes.search_probe_filtered_batch(qb, 1, similarity="one_minus_dist", filter=mask,
                                                                             approx=True),
        "approx with a cut above 1024": lambda: codes.search_probe_filtered_batch(qb, 600, filter=mask, approx=True),
        "nprobe=0": lambda: plain.search_probe_filtered(q1, 1, filter=mask, nprobe=0),
        "nprobe=-2": lambda: plain.search_probe_filtered_batch(qb, 1, filter=mask, nprobe=-2),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError):
            call()
        assert plain._corpus is None and codes._corpus is None, f"{name}: raised only after a build"


def test_signatures():
    from dewi.ivf import IVFIndex
    lead = ["self", "k", "eta", "entropy_pref", "candidates", "similarity", "filter", "nprobe", "widen", "approx", "rescore",
            "return_nprobe"]
    for name, first in (("search_probe_filtered", "query"), ("search_probe_filtered_batch", "queries"),
                        ("search_probe_filtered_device", "q_dev")):
        params = inspect.signature(getattr(IVFIndex, name)).parameters
        assert list(params) == lead[:1] + [first] + lead[1:], name
        assert params["filter"].default is inspect.Parameter.empty and params["filter"].kind is inspect.Parameter.KEYWORD_ONLY
        assert params["widen"].default is False and params["approx"].default is False and params["rescore"].default is True
        assert (params["k"].default, params["eta"].default, params["nprobe"].default) == (10, 0.5, None)
    # the existing entry points keep their rule: approx=True together with filter= raises
    with pytest.raises(ValueError):
        _index(int8_codes=True).search_batch(np.ones((1, 16), np.float32), 1, approx=True, filter=np.ones(2, bool))

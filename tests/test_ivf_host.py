"""Host side of the IVF index (no GPU): the additive exports (still exactly the header, ABI 6), the two size functions,
the approximate-backend stubs, and the argument checks of ``IVFIndex`` that need no device."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"
NEW_EXPORTS = {"dewi_ivf_buckets", "dewi_ivf_lists_bytes", "dewi_ivf_lists_build", "dewi_ivf_probe_group_bytes",
               "dewi_ivf_probe_bytes", "dewi_ivf_probe_prepare"}


def _header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(dewi_\w+)\s*\(", src))


def _period(dim):
    rb, tz = 4 * dim, 0
    while tz < 4 and (rb >> tz) % 2 == 0:
        tz += 1
    return 16 >> tz


def test_ivf_exports_equal_the_header():
    from dewi import _native as nat
    declared = _header_functions()
    assert NEW_EXPORTS <= declared
    assert set(nat.EXPORTED_SYMBOLS) == declared
    lib = nat.load_library(require_gpu=False)
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("dewi_")}
    assert exported == declared
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6


def test_ivf_buckets():
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    for dim in (64, 96, 768, 50, 129, 301, 5):
        assert lib.dewi_ivf_buckets(dim, 0) == _period(dim), dim
    assert lib.dewi_ivf_buckets(0, 0) == 0 and lib.dewi_ivf_buckets(64, 2) == 0


def test_ivf_lists_bytes_needs_no_device():
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    for n, dim, cells in ((20000, 64, 64), (20000, 50, 64), (20000, 129, 64), (1 << 20, 768, 1024), (600, 64, 512),
                          (100000, 129, 65536)):
        g = _period(dim)
        got = lib.dewi_ivf_lists_bytes(n, dim, 0, cells)
        assert got >= 4 * (cells * g + 1 + n), (n, dim, cells)
        assert got <= 4 * (2 * n + 2 * cells * g + 2), (n, dim, cells)   # the scratch stays below n + bins words
    for bad in ((0, 64, 0, 4), (100, 0, 0, 4), (100, 64, 2, 4), (100, 64, 0, 0), (100, 64, 0, -1), (100, 64, 0, 101),
                (1 << 20, 64, 0, 65537), (1 << 33, 64, 0, 4)):
        assert lib.dewi_ivf_lists_bytes(*bad) == 0, bad


def test_ivf_probe_bytes_needs_no_device():
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    for n, dim in ((20000, 64), (20000, 50), (1 << 20, 768), (600, 129)):
        for group in (1, 8, 32):
            one = lib.dewi_ivf_probe_group_bytes(n, dim, 0, group)
            assert one >= lib.dewi_query_filter_bytes(n, dim, 0, group) > 0, (n, dim, group)
            assert one >= 4 * (16 + 2 * n)
            for b in (1, group, group + 1, 4 * group):
                groups = (b + group - 1) // group
                got = lib.dewi_ivf_probe_bytes(n, dim, 0, b, group)
                assert got >= groups * one + 4 * (groups + b), (n, dim, group, b)
    for bad in ((0, 64, 0, 4, 8), (100, 0, 0, 4, 8), (100, 64, 2, 4, 8), (100, 64, 0, 0, 8), (100, 64, 0, 4, 0),
                (100, 64, 0, 4, 33), (100, 64, 0, 65536, 8)):
        assert lib.dewi_ivf_probe_bytes(*bad) == 0, bad
    assert lib.dewi_ivf_probe_group_bytes(100, 64, 0, 33) == 0


def test_ivf_entry_points_refuse_bf16_and_bad_shapes_before_any_device_work():
    import ctypes
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    cnt = (ctypes.c_int64 * 4)()
    assert lib.dewi_ivf_lists_build(1, 100, 64, 4, p, p, 1 << 20, None) == nat.ERR_UNSUPPORTED
    assert lib.dewi_ivf_lists_build(0, 100, 64, 101, p, p, 1 << 20, None) == nat.ERR_INVALID_ARG
    assert lib.dewi_ivf_lists_build(0, 100, 64, 4, p, p, 8, None) == nat.ERR_WORKSPACE
    assert lib.dewi_ivf_lists_build(0, 100, 64, 4, None, p, 1 << 20, None) == nat.ERR_INVALID_ARG
    assert lib.dewi_ivf_probe_prepare(1, 100, 64, p, 4, p, 2, 1, 8, p, 1 << 20, cnt, cnt, None) == nat.ERR_UNSUPPORTED
    assert lib.dewi_ivf_probe_prepare(0, 100, 64, p, 4, p, 2, 5, 8, p, 1 << 20, cnt, cnt, None) == nat.ERR_INVALID_ARG   # nprobe > cells
    assert lib.dewi_ivf_probe_prepare(0, 100, 64, p, 4, p, 2, 0, 8, p, 1 << 20, cnt, cnt, None) == nat.ERR_INVALID_ARG
    assert lib.dewi_ivf_probe_prepare(0, 100, 64, p, 4, p, 2, 1, 33, p, 1 << 20, cnt, cnt, None) == nat.ERR_INVALID_ARG
    assert lib.dewi_ivf_probe_prepare(0, 100, 64, p, 4, p, 2, 1, 8, p, 8, cnt, cnt, None) == nat.ERR_WORKSPACE
    with pytest.raises(NotImplementedError):
        nat.check(lib.dewi_ivf_lists_build(1, 100, 64, 4, p, p, 1 << 20, None))


def test_ann_stubs_stay_import_errors():
    from dewi.backends import FAISSIndex, HNSWIndex
    with pytest.raises(ImportError):
        FAISSIndex(dim=8)
    with pytest.raises(ImportError):
        HNSWIndex(dim=8)


def test_ivf_index_arguments():
    from dewi.backends import ExactIndex
    from dewi.ivf import IVFIndex, default_nlist, default_nprobe
    idx = IVFIndex(8)
    assert isinstance(idx, ExactIndex) and idx.space == "cosine" and idx.nlist is None and idx.nprobe is None
    assert idx.train_iters == 10 and idx.train_seed == 0 and idx.max_train_rows is None
    names = list(inspect.signature(IVFIndex.__init__).parameters)
    assert names[:8] == ["self", "dim", "space", "nlist", "nprobe", "train_iters", "train_seed", "max_train_rows"]
    for name in ("search", "search_batch"):
        params = inspect.signature(getattr(IVFIndex, name)).parameters
        parent = list(inspect.signature(getattr(ExactIndex, name)).parameters)
        assert list(params)[: len(parent)] == parent                   # the same leading parameters as ExactIndex
        assert list(params)[-1] == "nprobe" and params["nprobe"].kind is inspect.Parameter.KEYWORD_ONLY
    for bad in ({"nlist": 0}, {"nlist": 65537}, {"nprobe": 0}, {"nprobe": -3}, {"train_iters": -1}, {"max_train_rows": 0}):
        with pytest.raises(ValueError):
            IVFIndex(8, **bad)
    assert [default_nlist(n) for n in (1, 2, 100, 20000, 1 << 20, 1 << 30)] == [1, 1, 10, 141, 1024, 4096]
    assert [default_nprobe(n) for n in (1, 63, 64, 1024, 4096)] == [1, 1, 1, 16, 64]
    # nprobe is checked before anything is built (no device needed to be told it is wrong)
    from dewi.types import Payload
    idx.add_batch(["a", "b"], np.ones((2, 8), np.float32), [Payload(), Payload()])
    for call in (lambda: idx.search(np.ones(8, np.float32), nprobe=0), lambda: idx.search_batch(np.ones((1, 8), np.float32), nprobe=-1),
                 lambda: idx.probe(np.ones((1, 8), np.float32), 0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        idx.add("c", np.ones(7, np.float32), Payload())                 # add() is ExactIndex's


def test_ivf_is_not_part_of_the_reference_surface():
    import dewi
    from dewi import backends
    assert "IVFIndex" not in dewi.__all__ and not hasattr(backends, "IVFIndex")

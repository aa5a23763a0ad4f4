"""Subset selection, the host side (no GPU): the four new symbols in header / ``EXPORTED_SYMBOLS`` / the library's exports, the
argument errors of ``dewi_select_begin`` / ``_seed`` / ``_run`` (every one is raised before the first device call, so dummy
host pointers do), the workspace size, and the Python surface."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NEW = {"dewi_select_workspace_bytes", "dewi_select_begin", "dewi_select_seed", "dewi_select_run"}
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


def test_header_symbol_list_and_exports_agree():
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    declared = set(re.findall(r"\b(dewi_[a-z0-9_]+)\s*\(", header))
    assert NEW <= declared
    assert declared == set(nat.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("dewi_")}
    assert exported == declared, exported ^ declared
    assert lib_version(nat) == 6


def lib_version(nat):
    return nat.load_library(require_gpu=False).dewi_abi_version()


def begin(n=100, d=8, elem=0, mask=None, ws=P, nbytes=BIG):
    return lambda lib: lib.dewi_select_begin(n, d, elem, mask, ws, nbytes, None)


def seed(E=P, elem=0, n=100, d=8, rows=P, n_seeds=2, max_sim=INF, ws=P, nbytes=BIG):
    return lambda lib: lib.dewi_select_seed(E, elem, n, d, rows, n_seeds, max_sim, ws, nbytes, None)


def run(E=P, elem=0, n=100, d=8, rel=P, budget=5, lam=0.5, max_sim=INF, rows=P, gain=P, cnt=P, pen=None, owner=None, ws=P,
        nbytes=BIG):
    return lambda lib: lib.dewi_select_run(E, elem, n, d, rel, budget, lam, max_sim, 0, rows, gain, cnt, pen, owner, ws, nbytes, None)


NEED_100 = 2 * 256 * 8 + 256 + 9 * 128                 # keys, header, pen + owner + struck bytes of 128 (100 rounded up to 64s) rows

CASES = [
    ("begin: rows", begin(n=0), INVALID, "bad shape 0 x 8"),
    ("begin: dim", begin(d=-1), INVALID, "bad shape 100 x -1"),
    ("begin: rows 2^32", begin(n=1 << 32), UNSUPPORTED, "n_rows 4294967296 exceeds 2^32-1 rows per device"),
    ("begin: rows 2^31", begin(n=1 << 31), UNSUPPORTED, "n_rows 2147483648: a subset selection takes fewer than 2^31 rows"),
    ("begin: elem_type", begin(elem=3), INVALID, "unknown elem_type 3"),
    ("begin: null workspace", begin(ws=None), WORKSPACE, f"workspace {BIG} B < required {NEED_100} B"),
    ("begin: short workspace", begin(nbytes=NEED_100 - 1), WORKSPACE, f"workspace {NEED_100 - 1} B < required {NEED_100} B"),
    ("begin: order: the shape before the workspace", begin(n=0, ws=None), INVALID, "bad shape 0 x 8"),
    ("seed: null corpus", seed(E=None), INVALID, "null pointer"),
    ("seed: null rows", seed(rows=None), INVALID, "null pointer"),
    ("seed: negative count", seed(n_seeds=-1), INVALID, "n_seeds must not be negative (got -1)"),
    ("seed: max_sim NaN", seed(max_sim=NAN), INVALID, "max_sim is NaN"),
    ("seed: rows", seed(n=0), INVALID, "bad shape 0 x 8"),
    ("seed: elem_type", seed(elem=-1), INVALID, "unknown elem_type -1"),
    ("seed: short workspace", seed(nbytes=100), WORKSPACE, f"workspace 100 B < required {NEED_100} B"),
    ("seed: no seeds is no work", seed(rows=None, n_seeds=0), OK, None),
    ("seed: order: the arguments before no seeds", seed(rows=None, n_seeds=0, nbytes=0), WORKSPACE, f"workspace 0 B < required {NEED_100} B"),
    ("run: null corpus", run(E=None), INVALID, "null pointer"),
    ("run: null relevance", run(rel=None), INVALID, "null pointer"),
    ("run: null rows", run(rows=None), INVALID, "null pointer"),
    ("run: null gain", run(gain=None), INVALID, "null pointer"),
    ("run: null counter", run(cnt=None), INVALID, "null pointer"),
    ("run: rows", run(n=-5), INVALID, "bad shape -5 x 8"),
    ("run: dim", run(d=0), INVALID, "bad shape 100 x 0"),
    ("run: rows 2^31", run(n=(1 << 31) + 5), UNSUPPORTED, "n_rows 2147483653: a subset selection takes fewer than 2^31 rows"),
    ("run: elem_type", run(elem=2), INVALID, "unknown elem_type 2"),
    ("run: lambda above", run(lam=1.5), INVALID, "mmr_lambda 1.5 outside [0, 1]"),
    ("run: lambda below", run(lam=-0.25), INVALID, "mmr_lambda -0.25 outside [0, 1]"),
    ("run: lambda NaN", run(lam=NAN), INVALID, "mmr_lambda nan outside [0, 1]"),
    ("run: max_sim NaN", run(max_sim=NAN), INVALID, "max_sim is NaN"),
    ("run: null workspace", run(ws=None), WORKSPACE, f"workspace {BIG} B < required {NEED_100} B"),
    ("run: short workspace", run(nbytes=NEED_100 - 1), WORKSPACE, f"workspace {NEED_100 - 1} B < required {NEED_100} B"),
    ("run: budget 0 writes nothing", run(budget=0), OK, None),
    ("run: budget < 0", run(budget=-7), OK, None),
    ("run: order: the pointers before the shape", run(E=None, n=0), INVALID, "null pointer"),
    ("run: order: lambda before the shape", run(lam=2.0, n=0), INVALID, "mmr_lambda 2 outside [0, 1]"),
    ("run: order: the arguments before budget <= 0", run(budget=0, max_sim=NAN), INVALID, "max_sim is NaN"),
    ("run: order: the workspace before budget <= 0", run(budget=0, nbytes=8), WORKSPACE, f"workspace 8 B < required {NEED_100} B"),
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
    """4 KiB of keys, the header, then 9 bytes of state per row (rows rounded up to 64); 0 for a shape the calls refuse; it
    needs no device and does not depend on the width or the element type."""
    size = lib.dewi_select_workspace_bytes
    assert size(100, 8, 0) == NEED_100
    for n in (1, 64, 65, 2053, 1_000_000):
        want = 4096 + 256 + 9 * ((n + 63) // 64 * 64)
        assert size(n, 768, 0) == size(n, 50, 1) == want and want % 64 == 0
    for bad in [(0, 8, 0), (-1, 8, 0), (10, 0, 0), (10, 8, 2), (1 << 31, 8, 0)]:
        assert size(*bad) == 0
    assert size((1 << 31) - 1, 8, 0) > 9 * ((1 << 31) - 1)


def test_status_codes_become_exceptions(lib):
    from dewi import _native as nat
    with pytest.raises(ValueError, match="mmr_lambda 1.5 outside"):
        nat.check(run(lam=1.5)(lib))
    with pytest.raises(NotImplementedError, match="fewer than 2\\^31 rows"):
        nat.check(begin(n=1 << 31)(lib))


def test_python_signatures():
    from dewi._engine import DeviceCorpus, Int8Corpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    want = ["self", "budget", "mmr_lambda", "max_sim", "relevance", "filter", "seeds", "return_gain", "return_coverage"]
    for cls in (ExactIndex, DewiIndex, IVFIndex):
        sig = inspect.signature(cls.select_subset)
        assert list(sig.parameters) == want, cls.__name__
        assert sig.parameters["mmr_lambda"].default == 0.5 and sig.parameters["max_sim"].default is None
        assert sig.parameters["return_gain"].default is False and sig.parameters["return_coverage"].default is False
    assert IVFIndex.select_subset is ExactIndex.select_subset
    sig = inspect.signature(DeviceCorpus.select_subset_device)
    assert list(sig.parameters)[:7] == ["self", "budget", "mmr_lambda", "max_sim", "relevance", "mask", "seeds"]
    assert sig.parameters["mmr_lambda"].default == 0.5 and sig.parameters["max_sim"].default is None
    assert "select_subset_device" not in Int8Corpus._SERVED          # an int8-only corpus raises NotImplementedError


def test_l2_is_not_served():
    """Raised from the space alone: nothing is built, no device is needed."""
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    from dewi.types import Payload
    q = np.ones(4, np.float32)
    for idx in (ExactIndex(dim=4, space="l2"), IVFIndex(dim=4, space="l2"), DewiIndex(dim=4, space="l2")):
        idx.add("a", q, Payload())
        with pytest.raises(NotImplementedError, match="l2"):
            idx.select_subset(1)

"""Diverse search, the host side (no GPU): the two new symbols in header / ``EXPORTED_SYMBOLS`` / the library's exports, the
argument errors of ``dewi_diverse_rerank`` (every one is raised before the first device call, so dummy host pointers do), and
the Python surface."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NEW = {"dewi_diverse_workspace_bytes", "dewi_diverse_rerank"}
OK, INVALID, K_OOB, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -5

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer
INF = float("inf")
NAN = float("nan")


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


def test_abi_version_and_pool_limit(lib):
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    assert re.search(r"#define DEWI_ABI_VERSION 6\b", header)
    assert lib.dewi_abi_version() == 6 == nat.ABI_VERSION
    assert re.search(r"#define DEWI_DIVERSE_MAX_CANDIDATES 1024\b", header)
    assert nat.DIVERSE_MAX_CANDIDATES == 1024


def div(E=P, elem=0, n=100, d=8, cand=P, b=1, c=10, k=5, lam=0.5, max_sim=INF, ids=P, sc=P, mmr=None, ws=None, nbytes=0):
    return lambda lib: lib.dewi_diverse_rerank(E, elem, n, d, cand, b, c, k, 0.3, 0.0, lam, max_sim, 0, ids, sc, mmr, ws, nbytes,
                                               None)


CASES = [
    ("null corpus", div(E=None), INVALID, "null pointer"),
    ("null records", div(cand=None), INVALID, "null pointer"),
    ("null ids", div(ids=None), INVALID, "null pointer"),
    ("null scores", div(sc=None), INVALID, "null pointer"),
    ("rows", div(n=0), INVALID, "bad shape 0 x 8"),
    ("dim", div(d=0), INVALID, "bad shape 100 x 0"),
    ("rows 2^32", div(n=1 << 32), UNSUPPORTED, "n_rows 4294967296 exceeds 2^32-1 rows per device"),
    ("queries", div(b=0), INVALID, "non-positive size (0 queries, 10 candidates)"),
    ("candidates", div(c=0, k=0), INVALID, "non-positive size (1 queries, 0 candidates)"),
    ("elem_type", div(elem=2), INVALID, "unknown elem_type 2"),
    ("lambda above", div(lam=1.5), INVALID, "mmr_lambda 1.5 outside [0, 1]"),
    ("lambda below", div(lam=-0.25), INVALID, "mmr_lambda -0.25 outside [0, 1]"),
    ("lambda NaN", div(lam=NAN), INVALID, "mmr_lambda nan outside [0, 1]"),
    ("max_sim NaN", div(max_sim=NAN), INVALID, "max_sim is NaN"),
    ("k above the pool", div(k=11), K_OOB, "k 11 exceeds candidate count 10"),
    ("pool above the maximum", div(c=1025, k=5), UNSUPPORTED, "n_candidates 1025 exceeds the 1024 a diverse re-rank takes"),
    ("k <= 0 writes nothing", div(k=0), OK, None),
    ("k < 0", div(k=-3), OK, None),
    ("order: the pointers before the shape", div(E=None, n=0), INVALID, "null pointer"),
    ("order: lambda before k", div(lam=2.0, k=11), INVALID, "mmr_lambda 2 outside [0, 1]"),
    ("order: the arguments before k <= 0", div(k=0, max_sim=NAN), INVALID, "max_sim is NaN"),
    ("order: k before the pool limit", div(c=2000, k=2001), K_OOB, "k 2001 exceeds candidate count 2000"),
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


def test_workspace_is_empty_for_every_shape(lib):
    """The lazy re-rank keeps a query's state on chip: the size is 0, so DEWI_ERR_WORKSPACE (raised for a workspace below
    the size) cannot arise in this build and a NULL workspace is what callers pass."""
    for b, c, d in [(1, 1, 1), (1, 40, 768), (256, 1024, 4096), (37, 200, 50), (1, 1024, 100000)]:
        assert lib.dewi_diverse_workspace_bytes(b, c, d) == 0
    assert lib.dewi_diverse_workspace_bytes(0, -1, 0) == 0


def test_status_codes_become_exceptions(lib):
    from dewi import _native as nat
    with pytest.raises(ValueError, match="k 11 exceeds candidate count 10"):
        nat.check(div(k=11)(lib))
    with pytest.raises(NotImplementedError, match="n_candidates 1025 exceeds"):
        nat.check(div(c=1025)(lib))


def test_python_signatures():
    from dewi._engine import DeviceCorpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    want = ["k", "eta", "entropy_pref", "mmr_lambda", "candidates", "max_sim"]
    for cls in (ExactIndex, DewiIndex, IVFIndex):
        for name, first in (("search_diverse", "query"), ("search_diverse_batch", "queries")):
            params = list(inspect.signature(getattr(cls, name)).parameters)
            assert params == ["self", first] + want, (cls.__name__, name, params)
        for name in ("search", "search_batch") if cls is not IVFIndex else ():       # (IVFIndex's end in nprobe)
            assert list(inspect.signature(getattr(cls, name)).parameters)[-1] == "filter", (cls.__name__, name)
    assert IVFIndex.search_diverse is ExactIndex.search_diverse and IVFIndex.search_diverse_batch is ExactIndex.search_diverse_batch
    assert "search_diverse" in IVFIndex.__doc__
    sig = inspect.signature(DeviceCorpus.search_diverse_device)
    assert list(sig.parameters) == ["self", "q_dev", "k", "eta", "entropy_pref", "mmr_lambda", "candidates", "max_sim", "out_ids",
                                    "out_scores"]
    assert sig.parameters["mmr_lambda"].default == 0.5 and sig.parameters["max_sim"].default is None
    assert list(inspect.signature(DeviceCorpus.search_diverse).parameters)[:2] == ["self", "queries"]
    assert inspect.signature(ExactIndex.search_diverse).parameters["mmr_lambda"].default == 0.5
    assert inspect.signature(DewiIndex.search_diverse).parameters["eta"].default is None


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
            idx.search_diverse(q, k=1)
        with pytest.raises(NotImplementedError, match="l2"):
            idx.search_diverse_batch(q[None, :], k=1)

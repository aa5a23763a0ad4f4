"""Collapsed search, the host side (no GPU): the three new symbols in header / ``EXPORTED_SYMBOLS`` / the library's exports /
INTEGRATION.md, the argument errors of ``dewi_collapse_rerank`` and ``dewi_knn_candidates_filtered`` (every one is raised
before the first device call, so dummy host pointers do), ``group_labels`` / ``make_groups`` and the Python surface."""
import ctypes
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
NEW = {"dewi_collapse_workspace_bytes", "dewi_collapse_rerank", "dewi_knn_candidates_filtered"}
OK, INVALID, K_OOB, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -5

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_header_symbol_list_exports_and_integration_notes_agree():
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    declared = set(re.findall(r"\b(dewi_[a-z0-9_]+)\s*\(", header))
    assert NEW <= declared
    assert declared == set(nat.EXPORTED_SYMBOLS), declared ^ set(nat.EXPORTED_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("dewi_")}
    assert exported == declared, exported ^ declared
    notes = (REPO / "INTEGRATION.md").read_text()
    for name in NEW:
        assert f"`{name}`" in notes, name


def test_abi_version_and_pool_limit(lib):
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    assert re.search(r"#define DEWI_ABI_VERSION 6\b", header)
    assert lib.dewi_abi_version() == 6 == nat.ABI_VERSION
    assert re.search(r"#define DEWI_COLLAPSE_MAX_CANDIDATES 2048\b", header)
    assert nat.COLLAPSE_MAX_CANDIDATES == 2048


def test_workspace_is_empty_for_every_shape_and_needs_no_device(lib):
    for b, c in [(1, 1), (1, 40), (256, 2048), (37, 200), (0, -1), (1, 5000)]:
        assert lib.dewi_collapse_workspace_bytes(b, c) == 0


def col(cand=P, b=1, c=10, labels=P, n=100, off=0, k=5, m=1, ids=P, sc=P, hits=None, counts=None, ws=None, nbytes=0):
    return lambda lib: lib.dewi_collapse_rerank(cand, b, c, labels, n, off, k, m, 0.3, 0.0, ids, sc, hits, counts, ws, nbytes, None)


def rec(E=P, elem=0, n=100, d=8, filt=P, n_a=50, Q=P, b=1, dewi=P, ent=P, c=10, space=0, off=0, out=P, ws=P, nbytes=1 << 30):
    return lambda lib: lib.dewi_knn_candidates_filtered(E, elem, n, d, filt, n_a, Q, b, dewi, ent, c, space, off, out, ws, nbytes, None)


CASES = [
    ("collapse null records", col(cand=None), INVALID, "null pointer"),
    ("collapse null labels", col(labels=None), INVALID, "null pointer"),
    ("collapse null ids", col(ids=None), INVALID, "null pointer"),
    ("collapse null scores", col(sc=None), INVALID, "null pointer"),
    ("collapse queries", col(b=0), INVALID, "non-positive size (0 queries, 10 candidates)"),
    ("collapse candidates", col(c=0, k=0), INVALID, "non-positive size (1 queries, 0 candidates)"),
    ("collapse rows", col(n=0), INVALID, "n_rows must be positive (got 0)"),
    ("collapse per_group", col(m=0), INVALID, "per_group must be positive (got 0)"),
    ("collapse per_group < 0", col(m=-2), INVALID, "per_group must be positive (got -2)"),
    ("collapse k above the pool", col(k=11), K_OOB, "k 11 exceeds candidate count 10"),
    ("collapse pool above the maximum", col(c=2049), UNSUPPORTED, "n_candidates 2049 exceeds the 2048 a collapsed re-rank takes"),
    ("collapse k <= 0 writes nothing", col(k=0), OK, None),
    ("collapse k < 0", col(k=-3), OK, None),
    ("collapse order: the pointers before the shape", col(cand=None, n=0), INVALID, "null pointer"),
    ("collapse order: the arguments before k <= 0", col(k=0, m=0), INVALID, "per_group must be positive (got 0)"),
    ("collapse order: k before the pool limit", col(c=3000, k=3001), K_OOB, "k 3001 exceeds candidate count 3000"),
    ("records null corpus", rec(E=None), INVALID, "null embedding or query pointer"),
    ("records null queries", rec(Q=None), INVALID, "null embedding or query pointer"),
    ("records rows", rec(n=0), INVALID, "n_rows must be positive (got 0)"),
    ("records dim", rec(d=0), INVALID, "dim must be positive (got 0)"),
    ("records queries", rec(b=0), INVALID, "n_queries must be positive (got 0)"),
    ("records space", rec(space=2), INVALID, "unknown space 2"),
    ("records bf16", rec(elem=1), UNSUPPORTED, "filtered search serves fp32 corpora (bf16: not in this build)"),
    ("records elem_type", rec(elem=2), INVALID, "unknown elem_type 2"),
    ("records null filter", rec(filt=None), INVALID, "null filter pointer"),
    ("records n_allowed < 0", rec(n_a=-1), INVALID, "n_allowed -1 outside [0, 100]"),
    ("records n_allowed > n_rows", rec(n_a=101), INVALID, "n_allowed 101 outside [0, 100]"),
    ("records candidates", rec(c=0), INVALID, "n_candidates must be positive (got 0)"),
    ("records candidates 2049", rec(c=2049), UNSUPPORTED, "n_candidates 2049 exceeds the 2048 filtered candidate records take"),
    ("records null payload", rec(dewi=None), INVALID, "null payload or output pointer"),
    ("records null output", rec(out=None), INVALID, "null payload or output pointer"),
    ("records id_offset < 0", rec(off=-1), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 100 rows)"),
    ("records id_offset overflows int32", rec(off=2 ** 31 - 100), UNSUPPORTED,
     "global row ids must fit int32 (offset 2147483548 + 100 rows)"),
    ("records largest id_offset, empty list", rec(off=2 ** 31 - 101, n_a=0), OK, None),
    ("records empty list: nothing launched", rec(n_a=0, ws=None, nbytes=0), OK, None),
    ("records order: bf16 before the filter", rec(elem=1, filt=None), UNSUPPORTED, "filtered search serves fp32 corpora (bf16: not in this build)"),
    ("records order: the cut before the id range", rec(c=2049, off=-1), UNSUPPORTED,
     "n_candidates 2049 exceeds the 2048 filtered candidate records take"),
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


def test_status_codes_become_exceptions(lib):
    from dewi import _native as nat
    with pytest.raises(ValueError, match="k 11 exceeds candidate count 10"):
        nat.check(col(k=11)(lib))
    with pytest.raises(NotImplementedError, match="n_candidates 2049 exceeds"):
        nat.check(col(c=2049)(lib))
    with pytest.raises(NotImplementedError, match="bf16"):
        nat.check(rec(elem=1)(lib))


# ------------------------------------------------------------------------------------------------ group labels (host logic)
def test_group_labels_takes_the_four_input_forms():
    from dewi._engine import group_labels
    from dewi.backends import DuplicateGroups
    dup = DuplicateGroups(np.array([0, 0, 2, 3, 2], np.int64), np.array([2, 2, 2, 1, 2]), np.array([0, 0, 2, 3, 2]), 3)
    lab, n_groups = group_labels(dup, 5)
    assert lab.dtype == np.int32 and lab.tolist() == [0, 0, 2, 3, 2] and n_groups == 3
    lab, n_groups = group_labels(np.array([5, -1, 5, -7, 2 ** 31 - 1], np.int64), 5)
    assert lab.dtype == np.int32 and lab.tolist() == [5, -1, 5, -7, 2 ** 31 - 1] and n_groups == 4        # two ungrouped rows
    assert group_labels([3, 3, -1], 3)[0].tolist() == [3, 3, -1]
    lab, n_groups = group_labels(["a.org", "b.org", None, "a.org", ("x", 1)], 5)
    assert lab.tolist() == [0, 1, -1, 0, 2] and n_groups == 4
    assert group_labels(np.array(["u", "v", "u"], dtype=object), 3)[0].tolist() == [0, 1, 0]
    row_of = {"d0": 0, "d1": 1, "d2": 2, "d3": 3}
    lab, n_groups = group_labels({"d3": "s", "d1": "s", "d0": None}, 4, row_of)
    assert lab.tolist() == [-1, 0, -1, 0] and n_groups == 3
    assert group_labels([], 0)[0].shape == (0,)


def test_group_labels_refuses_bad_input():
    from dewi._engine import group_labels
    with pytest.raises(ValueError, match="length 4"):
        group_labels(["a", "b"], 4)
    with pytest.raises(ValueError, match=r"shape \(4,\)"):
        group_labels(np.zeros(5, np.int64), 4)
    with pytest.raises(ValueError, match=r"shape \(4,\)"):
        group_labels(np.zeros((4, 1), np.int32), 4)
    with pytest.raises(ValueError, match="int32"):
        group_labels(np.array([0, 2 ** 31], np.int64), 2)
    with pytest.raises(ValueError, match="int32"):
        group_labels(np.array([0, -2 ** 31 - 1], np.int64), 2)
    with pytest.raises(KeyError, match="nope"):
        group_labels({"d0": 1, "nope": 2}, 2, {"d0": 0, "d1": 1})
    with pytest.raises(ValueError, match="needs an index"):
        group_labels({"d0": 1}, 2)


class _StubCorpus:
    """What ``ExactIndex.make_groups`` asks of its corpus: labels in, a ``DeviceGroups`` out (no device)."""

    corpus_id = 41

    def __init__(self, n):
        self.n_rows = n

    def make_groups(self, labels):
        from dewi._engine import DeviceGroups, group_labels
        lab, n_groups = group_labels(labels, self.n_rows)
        return DeviceGroups(lab, n_groups, self.corpus_id, self.n_rows)

    def check_groups(self, groups):
        from dewi._engine import DeviceCorpus
        DeviceCorpus.check_groups(self, groups)


def _stubbed_index(n):
    from dewi.backends import ExactIndex
    idx = ExactIndex(dim=4)
    idx._doc_ids = [f"doc{i}" for i in range(n)]
    idx._corpus = _StubCorpus(n)
    idx._is_trained = True
    return idx


def test_make_groups_on_a_stubbed_index():
    from dewi._engine import DeviceGroups
    from dewi.backends import DuplicateGroups
    idx = _stubbed_index(4)
    g = idx.make_groups({"doc2": "site", "doc0": "site"})
    assert isinstance(g, DeviceGroups) and g.labels.tolist() == [0, -1, 0, -1] and g.n_groups == 3 and g.n_rows == 4
    assert g.corpus_id == 41 and len(g) == 3 and "3 groups" in repr(g)
    assert idx.make_groups(["x", "y", "x", None]).labels.tolist() == [0, 1, 0, -1]
    assert idx.make_groups(np.array([9, 9, -1, 4], np.int16)).labels.tolist() == [9, 9, -1, 4]
    assert idx.make_groups(DuplicateGroups(np.array([0, 1, 1, 3]), np.ones(4), np.arange(4), 3)).labels.tolist() == [0, 1, 1, 3]
    assert idx.make_groups(g) is g                                       # prepared labels pass through ...
    idx._corpus.corpus_id = 42                                           # ... until the corpus is another one
    with pytest.raises(ValueError, match="another corpus"):
        idx.make_groups(g)
    with pytest.raises(KeyError, match="doc9"):
        idx.make_groups({"doc9": 1})
    with pytest.raises(ValueError, match="length 4"):
        idx.make_groups(["a"])
    with pytest.raises(ValueError, match="int32"):
        idx.make_groups(np.array([0, 0, 0, 2 ** 40]))


def test_python_signatures():
    from dewi._engine import DeviceCorpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    want = ["k", "eta", "entropy_pref", "groups", "per_group", "candidates", "filter", "approx", "rescore", "widen", "return_hits"]
    for cls in (ExactIndex, DewiIndex, IVFIndex):
        for name, first in (("search_collapsed", "query"), ("search_collapsed_batch", "queries")):
            sig = inspect.signature(getattr(cls, name))
            assert list(sig.parameters)[:len(want) + 2] == ["self", first] + want, (cls.__name__, name)
            assert sig.parameters["groups"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["per_group"].default == 1
        assert callable(getattr(cls, "make_groups"))
    assert IVFIndex.search_collapsed is ExactIndex.search_collapsed and "search_collapsed" in IVFIndex.__doc__
    assert inspect.signature(DewiIndex.search_collapsed).parameters["eta"].default is None
    assert inspect.signature(ExactIndex.search_collapsed).parameters["eta"].default == 0.5
    sig = inspect.signature(DeviceCorpus.search_collapsed_device)
    assert list(sig.parameters) == ["self", "q_dev", "k", "eta", "entropy_pref", "groups", "per_group", "candidates", "filter",
                                    "approx", "rescore", "out_ids", "out_scores", "out_hits"]
    sig = inspect.signature(DeviceCorpus.search_collapsed)
    assert {"widen", "return_pool"} <= set(sig.parameters)
    assert list(inspect.signature(DeviceCorpus.candidates_filtered_device).parameters) == ["self", "q_dev", "n_candidates", "filter", "out"]
    # nothing existing changed its parameter list
    assert list(inspect.signature(ExactIndex.search).parameters)[-1] == "filter"
    assert list(inspect.signature(ExactIndex.search_diverse).parameters) == ["self", "query", "k", "eta", "entropy_pref", "mmr_lambda",
                                                                             "candidates", "max_sim"]


def test_argument_errors_of_the_index_methods_need_no_device():
    idx = _stubbed_index(4)
    q = np.ones((2, 4), np.float32)
    with pytest.raises(ValueError, match="per_group"):
        idx.search_collapsed_batch(q, groups=[0, 0, 1, 1], per_group=0)
    with pytest.raises(NotImplementedError, match="per-query"):
        idx.search_collapsed_batch(q, groups=[0, 0, 1, 1], filter=np.ones((2, 4), bool))

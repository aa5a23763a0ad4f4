"""Host logic of per-query filters (no GPU): the [B, N] mask forms and their errors, the stale-set bookkeeping, the
additive exports (still exactly the header) and the ABI version, which stays 6."""
import inspect
import re
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"
NEW_EXPORTS = {"dewi_query_filter_bytes", "dewi_query_filter_prepare", "dewi_knn_query_filtered_workspace_bytes",
               "dewi_knn_rerank_query_filtered"}


def _index(n=12, dim=8):
    from dewi.backends import ExactIndex
    from dewi.types import Payload
    idx = ExactIndex(dim)
    idx.add_batch([f"d{i}" for i in range(n)], np.ones((n, dim), np.float32), [Payload() for _ in range(n)])
    return idx


def test_query_filter_mask_forms():
    idx = _index()
    want = np.zeros((3, 12), bool)
    want[0, [0, 3, 11]] = True
    want[1, 5] = True
    got = idx.query_filter_masks(want)
    assert got.shape == (3, 12) and np.array_equal(got, want)
    assert np.array_equal(idx.query_filter_masks(want.tolist()), want)
    assert np.array_equal(idx.query_filter_masks(doc_ids=[["d0", "d11", "d3"], "d5", []]), want)
    assert np.array_equal(idx.query_filter_masks(rows=[[11, 0, 3, 3], np.array([5]), np.array([], np.int64)]), want)
    assert np.array_equal(idx.query_filter_masks(want[:1]), want[:1])


def test_query_filter_mask_errors():
    idx = _index()
    with pytest.raises(ValueError):
        idx.query_filter_masks(np.ones(12, bool))                     # one list: make_filter's form, not B lists
    with pytest.raises(ValueError):
        idx.query_filter_masks(np.ones((2, 11), bool))                # wrong length
    with pytest.raises(ValueError):
        idx.query_filter_masks(np.ones((0, 12), bool))                # no query
    with pytest.raises(ValueError):
        idx.query_filter_masks(np.ones((2, 12), np.int32))            # not boolean
    with pytest.raises(ValueError):
        idx.query_filter_masks(np.ones((2, 12), bool), rows=[[1]])    # two forms at once
    with pytest.raises(ValueError):
        idx.query_filter_masks()
    with pytest.raises(ValueError):
        idx.query_filter_masks(rows=[])
    with pytest.raises(KeyError):
        idx.query_filter_masks(doc_ids=[["d1"], ["missing"]])
    with pytest.raises(ValueError):
        idx.query_filter_masks(rows=[[0], [12]])
    with pytest.raises(ValueError):
        idx.query_filter_masks(rows=[[-1]])


def test_stale_query_filter_bookkeeping():
    from dewi._engine import DeviceCorpus, DeviceQueryFilters
    qf = DeviceQueryFilters(None, None, [5, 0, 10], n_union=12, corpus_id=7, n_rows=20)
    assert qf.n_queries == len(qf) == 3 and qf.n_allowed.tolist() == [5, 0, 10] and qf.n_union == 12
    assert "3 queries" in repr(qf) and "union 12" in repr(qf)
    ok = types.SimpleNamespace(corpus_id=7)
    DeviceCorpus.check_query_filters(ok, qf)
    DeviceCorpus.check_query_filters(ok, qf, 3)
    with pytest.raises(ValueError):
        DeviceCorpus.check_query_filters(ok, qf, 4)                   # n_queries != B
    with pytest.raises(ValueError):
        DeviceCorpus.check_query_filters(types.SimpleNamespace(corpus_id=8), qf)   # the corpus was rebuilt since
    with pytest.raises(TypeError):
        DeviceCorpus.check_query_filters(ok, np.ones((3, 20), bool))


def test_make_query_filters_on_both_indexes():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    for cls in (ExactIndex, DewiIndex):
        assert "make_query_filters" in cls.__dict__
        names = [p.name for p in inspect.signature(cls.make_query_filters).parameters.values()]
        assert names == ["self", "masks", "doc_ids", "rows"]
        for name in ("search", "search_batch"):                          # no new keyword: filter stays last
            assert list(inspect.signature(getattr(cls, name)).parameters)[-1] == "filter"


def test_query_filter_bytes_needs_no_device():
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    n = 1000
    one = lib.dewi_query_filter_bytes(n, 768, 0, 1)
    assert one >= lib.dewi_filter_bytes(n, 768, 0) + 4 * n            # the single-list buffer + one word per row
    assert lib.dewi_query_filter_bytes(n, 768, 0, 33) - lib.dewi_query_filter_bytes(n, 768, 0, 32) >= 4 * n   # a second word
    assert lib.dewi_query_filter_bytes(n, 301, 0, 8) > lib.dewi_query_filter_bytes(n, 768, 0, 8)   # residue buckets
    for bad in ((0, 768, 0, 4), (n, 0, 0, 4), (n, 8, 2, 4), (n, 768, 0, 0), (n, 768, 0, -1)):
        assert lib.dewi_query_filter_bytes(*bad) == 0, bad


def _header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(dewi_\w+)\s*\(", src))


def test_exports_still_equal_the_header():
    from dewi import _native as nat
    declared = _header_functions()
    assert NEW_EXPORTS <= declared
    assert set(nat.EXPORTED_SYMBOLS) == declared
    lib = nat.load_library(require_gpu=False)
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("dewi_")}
    assert exported == declared
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6

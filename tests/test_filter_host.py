"""Host logic of the filtered search (no GPU): mask / doc-id / row normalisation, the stale-filter bookkeeping, the new
signatures keeping the g6 leading parameters, and the library exporting exactly what the header declares."""
import inspect
import json
import re
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "dewi_hip.h"


def _index(n=12, dim=8):
    from dewi.backends import ExactIndex
    from dewi.types import Payload
    idx = ExactIndex(dim)
    idx.add_batch([f"d{i}" for i in range(n)], np.ones((n, dim), np.float32), [Payload() for _ in range(n)])
    return idx


def test_filter_mask_forms():
    idx = _index()
    want = np.zeros(12, bool)
    want[[0, 3, 11]] = True
    assert np.array_equal(idx.filter_mask(want), want)
    assert np.array_equal(idx.filter_mask(doc_ids=["d0", "d11", "d3"]), want)
    assert np.array_equal(idx.filter_mask(doc_ids="d3"), np.arange(12) == 3)
    assert np.array_equal(idx.filter_mask(rows=[11, 0, 3, 3]), want)
    assert np.array_equal(idx.filter_mask(rows=np.array([], np.int64)), np.zeros(12, bool))
    assert np.array_equal(idx.filter_mask(doc_ids=[]), np.zeros(12, bool))


def test_filter_mask_errors():
    idx = _index()
    with pytest.raises(ValueError):
        idx.filter_mask(np.ones(11, bool))                       # wrong length
    with pytest.raises(ValueError):
        idx.filter_mask(np.ones(12, np.int32))                   # not boolean
    with pytest.raises(ValueError):
        idx.filter_mask(np.ones(12, bool), rows=[1])             # two forms at once
    with pytest.raises(ValueError):
        idx.filter_mask()
    with pytest.raises(KeyError):
        idx.filter_mask(doc_ids=["d1", "missing"])
    with pytest.raises(ValueError):
        idx.filter_mask(rows=[12])
    with pytest.raises(ValueError):
        idx.filter_mask(rows=[-1])
    with pytest.raises(ValueError):
        idx.filter_mask(rows=[0.5])


def test_unprepared_filter_arguments():
    from dewi.backends import filter_kwargs
    assert set(filter_kwargs(np.ones(4, bool))) == {"mask"}
    assert set(filter_kwargs([True, False])) == {"mask"}
    assert filter_kwargs("d1") == {"doc_ids": ["d1"]}
    assert filter_kwargs(["d1", "d2"]) == {"doc_ids": ["d1", "d2"]}
    r = filter_kwargs([3, 1])["rows"]
    assert r.dtype == np.int64 and r.tolist() == [3, 1]
    assert set(filter_kwargs(np.arange(3))) == {"rows"}
    assert filter_kwargs([])["rows"].size == 0


def test_stale_filter_bookkeeping():
    from dewi._engine import DeviceCorpus, DeviceFilter
    f = DeviceFilter(None, 5, corpus_id=7, n_rows=10)
    assert len(f) == 5 and "5 of 10" in repr(f)
    DeviceCorpus.check_filter(types.SimpleNamespace(corpus_id=7), f)
    with pytest.raises(ValueError):
        DeviceCorpus.check_filter(types.SimpleNamespace(corpus_id=8), f)     # the corpus was rebuilt since
    with pytest.raises(TypeError):
        DeviceCorpus.check_filter(types.SimpleNamespace(corpus_id=7), np.ones(10, bool))


def _params(fn):
    return list(inspect.signature(fn).parameters.values())


def test_filter_signatures_keep_g6_leading_parameters(golden_dir):
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    surface = json.loads((golden_dir / "g6_api_surface.json").read_text())
    text = json.dumps(surface)
    for cls in (ExactIndex, DewiIndex):
        for name in ("search", "search_batch"):
            ps = _params(getattr(cls, name))
            assert ps[-1].name == "filter" and ps[-1].default is None, (cls.__name__, name)
        assert "make_filter" in cls.__dict__
    # the reference's leading parameters of search are still first (the g6 test checks all of them)
    for cls in (ExactIndex, DewiIndex):
        names = [p.name for p in _params(cls.search)]
        assert names[:4] == ["self", "query", "k", "eta"]
    assert "search" in text


def _header_functions():
    src = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(dewi_\w+)\s*\(", src))


def test_library_exports_exactly_the_header():
    from dewi import _native as nat
    declared = _header_functions()
    assert {"dewi_filter_bytes", "dewi_filter_prepare", "dewi_knn_filtered_workspace_bytes", "dewi_knn_rerank_filtered"} <= declared
    assert set(nat.EXPORTED_SYMBOLS) == declared
    lib = nat.load_library(require_gpu=False)
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6
    out = subprocess.run(["nm", "-D", "--defined-only", str(nat.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("dewi_")}
    assert exported == declared


def test_filter_bytes_needs_no_device():
    from dewi import _native as nat
    lib = nat.load_library(require_gpu=False)
    n = 1000
    whole = lib.dewi_filter_bytes(n, 768, 0)
    odd = lib.dewi_filter_bytes(n, 301, 0)
    assert whole >= 4 * (16 + n) and odd > whole                  # 4 residue buckets of scratch counts for dim 301
    assert lib.dewi_filter_bytes(0, 768, 0) == 0 and lib.dewi_filter_bytes(n, 0, 0) == 0 and lib.dewi_filter_bytes(n, 8, 2) == 0

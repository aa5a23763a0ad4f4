"""The int8 route without a GPU: the argument errors of its five entry points (a table in the form of
test_abi_errors_host.py: dummy pointers, exact code and message, one ``order`` case per entry point — no case gets as far as
the device), the workspace size (which needs no device), and the ``ValueError``s of the Python layer."""
import ctypes
import inspect

import numpy as np
import pytest

OK, INVALID, K_OOB, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -5
ROWS_2_32 = "n_rows 4294967296 exceeds 2^32-1 rows per device"
BIG = 1 << 32

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer


def quant(E=P, n=10, d=16, codes=P, scales=P):
    return lambda lib: lib.dewi_quantize_rows_i8(E, n, d, codes, scales, None)


def prep(Q=P, b=2, d=16, codes=P, scales=P, qn=None):
    return lambda lib: lib.dewi_prepare_queries_i8(Q, b, d, codes, scales, qn, None)


def cand(codes=P, scales=P, n=10, d=16, Q=P, b=1, dewi=P, c=4, id_offset=0, out=P, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_candidates_i8(codes, scales, n, d, Q, b, dewi, P, c, id_offset, out, ws, nbytes, None)


def rescore(E=P, n=10, d=16, Q=P, b=1, recs=P, c=4):
    return lambda lib: lib.dewi_rescore_candidates_f32(E, n, d, Q, b, recs, c, 0, None)


CASES = [
    # ---- dewi_quantize_rows_i8
    ("quantize empty", quant(n=0), OK, None),
    ("quantize n_rows", quant(n=-1), INVALID, "n_rows must be positive (got -1)"),
    ("quantize rows", quant(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("quantize dim 0", quant(d=0), INVALID, "dim must be positive (got 0)"),
    ("quantize dim % 16", quant(d=24), UNSUPPORTED, "dim 24: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("quantize dim > 4096", quant(d=4112), UNSUPPORTED, "dim 4112: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("quantize null", quant(scales=None), INVALID, "null pointer"),
    ("quantize alignment", quant(codes=P + 8), INVALID, "the codes must be 16-byte aligned"),
    ("quantize order: shape before null", quant(E=None, d=24), UNSUPPORTED,
     "dim 24: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    # ---- dewi_prepare_queries_i8
    ("prepare i8 n_queries", prep(b=0), INVALID, "n_queries must be positive (got 0)"),
    ("prepare i8 dim", prep(d=40), UNSUPPORTED, "dim 40: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("prepare i8 null", prep(Q=None), INVALID, "null pointer"),
    ("prepare i8 alignment", prep(qn=P + 4), INVALID, "the normalised queries must be 16-byte aligned"),
    ("prepare i8 order: n_queries before dim", prep(b=-2, d=40), INVALID, "n_queries must be positive (got -2)"),
    # ---- dewi_knn_candidates_i8
    ("candidates i8 null codes", cand(codes=None), INVALID, "null codes, scales or query pointer"),
    ("candidates i8 null Q", cand(Q=None), INVALID, "null codes, scales or query pointer"),
    ("candidates i8 n_rows", cand(n=0), INVALID, "n_rows must be positive (got 0)"),
    ("candidates i8 rows", cand(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("candidates i8 dim % 16", cand(d=8), UNSUPPORTED, "dim 8: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("candidates i8 dim > 4096", cand(d=8192), UNSUPPORTED, "dim 8192: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("candidates i8 n_queries", cand(b=0), INVALID, "n_queries must be positive (got 0)"),
    ("candidates i8 c <= 0", cand(c=0), INVALID, "n_candidates must be positive (got 0)"),
    ("candidates i8 c > 1024", cand(n=5000, c=1025), UNSUPPORTED, "n_candidates 1025 exceeds the 1024 the int8 route takes"),
    ("candidates i8 null payload", cand(dewi=None), INVALID, "null payload or output pointer"),
    ("candidates i8 null out", cand(out=None), INVALID, "null payload or output pointer"),
    ("candidates i8 alignment", cand(codes=P + 4), INVALID, "the codes must be 16-byte aligned"),
    ("candidates i8 id_offset", cand(id_offset=-1), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("candidates i8 workspace", cand(nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("candidates i8 null workspace", cand(ws=None), WORKSPACE, "workspace 1048576 B < required 256 B"),
    ("candidates i8 c > n_rows is padding, not an error", cand(n=3, c=8, nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("candidates i8 order: the shape before the cut", cand(d=24, c=2000), UNSUPPORTED,
     "dim 24: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("candidates i8 order: the cut before the null payload", cand(c=2000, dewi=None), UNSUPPORTED,
     "n_candidates 2000 exceeds the 1024 the int8 route takes"),
    # ---- dewi_rescore_candidates_f32
    ("rescore null", rescore(recs=None), INVALID, "null pointer"),
    ("rescore n_rows", rescore(n=0), INVALID, "n_rows must be positive (got 0)"),
    ("rescore rows", rescore(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("rescore dim % 4", rescore(d=18), UNSUPPORTED, "dim 18: the int8 route takes dim % 4 == 0 up to 4096 columns"),
    ("rescore n_queries", rescore(b=0), INVALID, "n_queries must be positive (got 0)"),
    ("rescore c > 1024", rescore(c=1025), UNSUPPORTED, "n_candidates 1025 exceeds the 1024 the int8 route takes"),
    ("rescore alignment", rescore(E=P + 4), INVALID, "the rows must be 16-byte aligned"),
    ("rescore order: null before shape", rescore(Q=None, n=0), INVALID, "null pointer"),
]


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,call,code,message", CASES, ids=[c[0] for c in CASES])
def test_abi_argument_error(lib, name, call, code, message):
    from dewi import _native as nat
    rc = call(lib)
    got = nat.last_error()
    print(f"{name}: rc {rc}, {got!r}")
    assert rc == code, (name, rc, got)
    if message is not None:
        assert got == message, name


def test_workspace_size_needs_no_device(lib):
    size = lib.dewi_knn_i8_workspace_bytes
    for bad in ((0, 16, 1, 4), (BIG, 16, 1, 4), (10, 24, 1, 4), (10, 4112, 1, 4), (10, 0, 1, 4), (10, 16, 0, 4), (10, 16, 1, 0),
                (5000, 16, 1, 1025)):
        assert size(*bad) == 0, bad
    # one workgroup, one sorted list of c keys per query (c <= 64); c > n_rows is sized for the rows there are
    assert size(10, 16, 1, 4) == 256 and size(10, 16, 3, 64) == 256 and size(3, 16, 1, 8) == 256
    # dense keys above 256 candidates: one key per row and query
    assert size(100000, 768, 4, 257) == 4 * 100000 * 8
    # lists: 256 workgroups at most; 8 waves each above 64 candidates
    assert size(1 << 20, 768, 1, 20) == 256 * 20 * 8
    assert size(1 << 20, 768, 2, 200) == 2 * 256 * 8 * 200 * 8
    assert size(1 << 20, 768, 1, 20) == size((1 << 32) - 1, 768, 1, 20)


def test_status_codes_become_exceptions(lib):
    from dewi import _native as nat
    with pytest.raises(NotImplementedError, match="dim 24: the int8 route"):
        nat.check(quant(d=24)(lib))
    with pytest.raises(ValueError, match="n_candidates must be positive"):
        nat.check(cand(c=0)(lib))
    assert nat.I8_MAX_CANDIDATES == 1024 and nat.I8_MAX_DIM == 4096


# ---------------------------------------------------------------------------------------------- the Python layer
def test_constructor_value_errors():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    assert ExactIndex(32, int8_shadow=True)._int8_shadow and not ExactIndex(32)._int8_shadow
    assert DewiIndex(32, use_ann=False, int8_shadow=True)._backend._int8_shadow
    assert not DewiIndex(32, use_ann=False)._backend._int8_shadow
    with pytest.raises(ValueError, match="cosine"):
        ExactIndex(32, space="l2", int8_shadow=True)
    with pytest.raises(ValueError, match="cosine"):
        DewiIndex(32, space="l2", use_ann=False, int8_shadow=True)
    for dim in (8, 24, 4112):
        with pytest.raises(ValueError, match="dim % 16"):
            ExactIndex(dim, int8_shadow=True)
    with pytest.raises(ValueError, match="IVFIndex does not take int8_shadow"):
        IVFIndex(32, int8_shadow=True)
    assert IVFIndex(32, int8_shadow=False)._int8_shadow is False


def test_approx_argument_errors_come_before_any_build():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    q = np.zeros((1, 32), np.float32)
    plain, shadowed = ExactIndex(32), ExactIndex(32, int8_shadow=True)
    with pytest.raises(ValueError, match="int8_shadow=True"):
        plain.search_batch(q, 5, approx=True)
    with pytest.raises(ValueError, match="int8_shadow=True"):
        plain.search(q[0], 5, approx=True)
    with pytest.raises(ValueError, match="does not take a filter"):
        shadowed.search_batch(q, 5, approx=True, filter=np.ones(4, bool))
    with pytest.raises(ValueError, match="similarity transform"):
        shadowed.search_batch(q, 5, candidates=5, similarity="one_minus_dist", approx=True)
    with pytest.raises(ValueError, match="int8_shadow=True"):
        plain.search_diverse_approx_batch(q, 5)
    with pytest.raises(ValueError, match="int8_shadow=True"):
        IVFIndex(32).search_batch(q, 5, approx=True)
    # None: "the index has an int8 shadow", where the route serves the call
    assert shadowed._use_approx(None, "ip", None, 10, None) is True
    assert shadowed._use_approx(None, "ip", None, 512, None) is True and shadowed._use_approx(None, "ip", None, 513, None) is False
    assert shadowed._use_approx(None, "ip", None, 10, None, 4) is True and shadowed._use_approx(None, "ip", None, 10, None, 5) is False
    assert shadowed._use_approx(True, "ip", None, 10, None, 64) is True          # asked for: any batch
    assert shadowed._use_approx(None, "ip", object(), 10, None) is False
    assert shadowed._use_approx(None, "one_minus_dist", None, 10, 10) is False
    assert shadowed._use_approx(False, "ip", None, 10, None) is False
    assert plain._use_approx(None, "ip", None, 10, None) is False and plain._use_approx(False, "ip", None, 10, None) is False
    # the facade hands the keywords through only when they are set
    d = DewiIndex(32, use_ann=False)
    assert d._approx_kwargs(None, True) == {} and d._approx_kwargs(True, False) == {"approx": True, "rescore": False}


def test_cut_rule_and_shape_rule():
    from dewi._engine import approx_cut, check_int8_shape
    assert approx_cut(10, None, 1000) == 20 and approx_cut(10, None, 15) == 15 and approx_cut(10, 64, 1000) == 64
    assert approx_cut(512, None, 5000) == 1024 and approx_cut(600, None, 1000) == 1000
    with pytest.raises(ValueError, match="at most 1024"):
        approx_cut(513, None, 5000)
    with pytest.raises(ValueError, match="at most 1024"):
        approx_cut(10, 1025, 5000)
    with pytest.raises(ValueError, match="k = 30 exceeds the cut of 20"):
        approx_cut(30, 20, 5000)
    with pytest.raises(ValueError, match="k = 11 exceeds the cut of 10"):
        approx_cut(11, None, 10)
    check_int8_shape("cosine", False, 768)
    for args in (("l2", False, 768), ("cosine", True, 768), ("cosine", False, 772), ("cosine", False, 8192)):
        with pytest.raises(ValueError):
            check_int8_shape(*args)


def test_signatures():
    from dewi._engine import DeviceCorpus, Int8Corpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    for cls in (ExactIndex, DewiIndex, IVFIndex):
        for name in ("search", "search_batch"):
            ps = inspect.signature(getattr(cls, name)).parameters
            assert ps["approx"].default is None and ps["approx"].kind is inspect.Parameter.KEYWORD_ONLY, (cls.__name__, name)
            assert ps["rescore"].default is True and ps["rescore"].kind is inspect.Parameter.KEYWORD_ONLY, (cls.__name__, name)
    for cls in (ExactIndex, DewiIndex):
        for name, first in (("search_diverse_approx", "query"), ("search_diverse_approx_batch", "queries")):
            assert list(inspect.signature(getattr(cls, name)).parameters) == [
                "self", first, "k", "eta", "entropy_pref", "mmr_lambda", "candidates", "max_sim", "rescore"]
    assert list(inspect.signature(DeviceCorpus.search_approx_device).parameters) == [
        "self", "q_dev", "k", "eta", "entropy_pref", "candidates", "rescore", "out_ids", "out_scores"]
    for name in ("enable_int8_shadow", "to_int8", "candidates_i8_device", "rescore_candidates_device", "search_approx",
                 "search_diverse_approx_device", "search_diverse_approx"):
        assert callable(getattr(DeviceCorpus, name))
    assert issubclass(Int8Corpus, DeviceCorpus)
    assert inspect.signature(Int8Corpus.search_approx).parameters["rescore"].default is False


def test_a_standalone_int8_corpus_refuses_everything_else():
    from dewi._engine import Int8Corpus
    c = object.__new__(Int8Corpus)
    for name in ("search", "search_device", "search_diverse", "range_search_device", "remove_rows", "put_rows", "to_bf16",
                 "enable_bf16_shadow", "enable_int8_shadow", "to_int8", "make_filter", "candidates_device",
                 "rescore_candidates_device", "near_duplicates_device"):
        with pytest.raises(NotImplementedError, match="stand-alone int8 corpus"):
            getattr(c, name)
    assert callable(c.search_approx) and callable(c.search_approx_device)

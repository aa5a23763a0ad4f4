"""CPU: the int8 route over allow-lists and IVF probes — every argument error of the three new entry points,
raised with no device (the pattern of tests/test_abi_errors_host.py: a dummy non-null host pointer stands for a device
pointer, a call that fails here has enqueued nothing), the size function, and the Python argument checks."""
import ctypes
import inspect

import numpy as np
import pytest

OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -5
BIG = 1 << 32
_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer
DIM_TEXT = "the int8 route takes dim % 16 == 0 up to 4096 columns"


def counts(*v):
    return (ctypes.c_int64 * len(v))(*v)


def one(codes=P, scales=P, n=10, d=16, filt=P, n_a=10, Q=P, b=1, dewi=P, ent=P, c=4, off=0, out=P, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_candidates_i8_filtered(codes, scales, n, d, filt, n_a, Q, b, dewi, ent, c, off, out, ws, nbytes,
                                                           None)


def per(codes=P, scales=P, n=10, d=16, filt=P, n_u=8, n_a=(8, 8), Q=P, b=2, dewi=P, ent=P, c=4, off=0, out=P, ws=P,
        nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_candidates_i8_query_filtered(codes, scales, n, d, filt, n_u, counts(*n_a) if n_a else None, Q, b,
                                                                 dewi, ent, c, off, out, ws, nbytes, None)


def shared_cases(name, f):
    """The checks both entry points make, in the order they make them."""
    return [
        (f"{name} null codes", f(codes=None), INVALID, "null codes, scales or query pointer"),
        (f"{name} null scales", f(scales=None), INVALID, "null codes, scales or query pointer"),
        (f"{name} null queries", f(Q=None), INVALID, "null codes, scales or query pointer"),
        (f"{name} n_rows 0", f(n=0), INVALID, "n_rows must be positive (got 0)"),
        (f"{name} n_rows 2^32", f(n=BIG), UNSUPPORTED, "n_rows 4294967296 exceeds 2^32-1 rows per device"),
        (f"{name} dim 0", f(d=0), INVALID, "dim must be positive (got 0)"),
        (f"{name} dim % 16", f(d=24), UNSUPPORTED, f"dim 24: {DIM_TEXT}"),
        (f"{name} dim > 4096", f(d=4112), UNSUPPORTED, f"dim 4112: {DIM_TEXT}"),
        (f"{name} n_queries 0", f(b=0), INVALID, "n_queries must be positive (got 0)"),
        (f"{name} n_candidates 0", f(c=0), INVALID, "n_candidates must be positive (got 0)"),
        (f"{name} n_candidates 1025", f(c=1025), UNSUPPORTED, "n_candidates 1025 exceeds the 1024 the int8 route takes"),
        (f"{name} null payload", f(dewi=None), INVALID, "null payload or output pointer"),
        (f"{name} null ent", f(ent=None), INVALID, "null payload or output pointer"),
        (f"{name} null out", f(out=None), INVALID, "null payload or output pointer"),
        (f"{name} null filter", f(filt=None), INVALID, "null filter pointer"),
        (f"{name} codes alignment", f(codes=P + 8), INVALID, "the codes must be 16-byte aligned"),
        (f"{name} queries alignment", f(Q=P + 4), INVALID, "the queries must be 16-byte aligned"),
        (f"{name} id_offset negative", f(off=-1), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 10 rows)"),
        (f"{name} id_offset int32", f(off=(1 << 31) - 10), UNSUPPORTED, "global row ids must fit int32 (offset 2147483638 + 10 rows)"),
        (f"{name} order: pointers before shape", f(codes=None, n=0, d=24), INVALID, "null codes, scales or query pointer"),
        (f"{name} order: shape before the candidates", f(d=24, c=0), UNSUPPORTED, f"dim 24: {DIM_TEXT}"),
        (f"{name} order: payload before the filter", f(dewi=None, filt=None), INVALID, "null payload or output pointer"),
        (f"{name} order: filter before alignment", f(filt=None, codes=P + 8), INVALID, "null filter pointer"),
    ]


CASES = shared_cases("one", one) + shared_cases("per", per) + [
    ("one n_allowed above", one(n_a=11), INVALID, "n_allowed 11 outside [0, 10]"),
    ("one n_allowed negative", one(n_a=-1), INVALID, "n_allowed -1 outside [0, 10]"),
    ("one empty list", one(n_a=0, ws=None, nbytes=0), OK, None),
    ("one workspace", one(nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("one null workspace", one(ws=None), WORKSPACE, "workspace 1048576 B < required 256 B"),
    ("one order: id_offset before n_allowed", one(off=-1, n_a=11), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("one order: n_allowed before the workspace", one(n_a=11, nbytes=16), INVALID, "n_allowed 11 outside [0, 10]"),
    ("per null counts", per(n_a=None), INVALID, "null count pointer"),
    ("per n_queries", per(b=65536), INVALID, "n_queries 65536 outside [1, 65535]"),
    ("per n_union above", per(n_u=11), INVALID, "n_union 11 outside [0, 10]"),
    ("per n_union negative", per(n_u=-2), INVALID, "n_union -2 outside [0, 10]"),
    ("per count above the union", per(n_a=(8, 9)), INVALID, "query 1: n_allowed 9 outside [0, 8]"),
    ("per count negative", per(n_a=(-1, 8)), INVALID, "query 0: n_allowed -1 outside [0, 8]"),
    ("per short list", per(n_a=(8, 3)), INVALID, "query 1: 3 allowed rows < the batch's cut 4 (search it on its own filter)"),
    ("per empty list", per(n_a=(0, 8)), INVALID, "query 0: 0 allowed rows < the batch's cut 4 (search it on its own filter)"),
    ("per empty union", per(n_u=0, n_a=(0, 0)), INVALID, "query 0: 0 allowed rows < the batch's cut 4 (search it on its own filter)"),
    ("per workspace", per(nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("per order: counts pointer before n_queries", per(n_a=None, b=65536), INVALID, "null count pointer"),
    ("per order: n_union before the counts", per(n_u=11, n_a=(3, 12)), INVALID, "n_union 11 outside [0, 10]"),
    ("per order: the first bad query wins", per(n_a=(3, 9)), INVALID,
     "query 0: 3 allowed rows < the batch's cut 4 (search it on its own filter)"),
    ("per order: the counts before the workspace", per(n_a=(8, 3), nbytes=16), INVALID,
     "query 1: 3 allowed rows < the batch's cut 4 (search it on its own filter)"),
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


def test_size_function_needs_no_device(lib):
    size, plain = lib.dewi_knn_i8_filtered_workspace_bytes, lib.dewi_knn_i8_workspace_bytes
    for bad in ((0, 768, 1, 20), (-1, 768, 1, 20), (BIG, 768, 1, 20), (100, 0, 1, 20), (100, 24, 1, 20), (100, 4112, 1, 20),
                (100, 768, 0, 20), (100, 768, 1, 0), (100, 768, 1, 1025)):
        assert size(*bad) == 0, bad
    for shape in ((1, 16, 1, 1), (70, 768, 4, 1024), (4099, 768, 37, 257), (1 << 20, 768, 1, 20), (4099, 48, 9, 64)):
        assert size(*shape) == plain(*shape) > 0 and size(*shape) % 256 == 0, shape
    # keys of every query: lists per workgroup (c <= 64), per wave (c <= 256), one per list position above
    # 4099 rows of 48 units, 8 in flight: 513 steps, 17 workgroups, one sorted list of 20 keys each
    assert size(4099, 768, 1, 20) == 2816 == (17 * 20 * 8 + 255) // 256 * 256
    assert size(1000, 768, 3, 300) == 24064 == (3 * 1000 * 8 + 255) // 256 * 256


def test_exports_and_status_codes(lib):
    from dewi import _native as nat
    for name in ("dewi_knn_i8_filtered_workspace_bytes", "dewi_knn_candidates_i8_filtered", "dewi_knn_candidates_i8_query_filtered"):
        assert name in nat.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.dewi_abi_version() == nat.ABI_VERSION == 6
    with pytest.raises(NotImplementedError, match="dim % 16"):
        nat.check(one(d=24)(lib))
    with pytest.raises(ValueError, match="search it on its own filter"):
        nat.check(per(n_a=(8, 3))(lib))


# ---------------------------------------------------------------------------------------------- the Python layer
def test_ivf_constructor():
    from dewi.ivf import IVFIndex
    assert IVFIndex(32, int8_codes=True)._int8_codes is True and IVFIndex(32)._int8_codes is False
    assert IVFIndex(32, int8_codes=True)._int8_shadow is False
    with pytest.raises(ValueError, match="cosine"):
        IVFIndex(32, space="l2", int8_codes=True)
    for dim in (8, 24, 4112):
        with pytest.raises(ValueError, match="dim % 16"):
            IVFIndex(dim, int8_codes=True)
    with pytest.raises(ValueError, match="IVFIndex does not take int8_shadow"):
        IVFIndex(32, int8_shadow=True)
    with pytest.raises(ValueError, match="IVFIndex does not take int8_shadow"):
        IVFIndex(32, int8_shadow=True, int8_codes=True)
    assert IVFIndex(32, nlist=4, nprobe=2, int8_codes=True).nprobe == 2


def test_pinned_errors_are_still_raised_before_any_build():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    q = np.zeros((1, 32), np.float32)
    plain, shadowed = ExactIndex(32), ExactIndex(32, int8_shadow=True)
    with pytest.raises(ValueError, match="does not take a filter"):
        shadowed.search_batch(q, 5, approx=True, filter=np.ones(4, bool))
    with pytest.raises(ValueError, match="search_approx_filtered"):
        shadowed.search_batch(q, 5, approx=True, filter=np.ones(4, bool))
    assert shadowed._use_approx(None, "ip", object(), 10, None) is False            # None + filter: the exact path
    with pytest.raises(ValueError, match="int8_shadow=True"):
        plain.search_approx_filtered_batch(q, 5, filter=np.ones(4, bool))
    with pytest.raises(ValueError, match="int8_shadow=True"):
        DewiIndex(32, use_ann=False).search_approx_filtered(q[0], 5, filter=np.ones(4, bool))
    with pytest.raises(ValueError, match="needs a filter"):
        shadowed.search_approx_filtered_batch(q, 5, filter=None)
    no_codes, codes = IVFIndex(32), IVFIndex(32, int8_codes=True)
    for call in (lambda: no_codes.search_batch(q, 5, approx=True), lambda: no_codes.search(q[0], 5, approx=True)):
        with pytest.raises(ValueError, match="int8_shadow=True"):
            call()
        with pytest.raises(ValueError, match="int8_codes=True"):
            call()
    with pytest.raises(ValueError, match="does not take a filter"):
        codes.search_batch(q, 5, approx=True, filter=np.ones(4, bool))
    with pytest.raises(ValueError, match="similarity transform"):
        codes.search_batch(q, 5, candidates=5, similarity="one_minus_dist", approx=True)
    # None: the int8 probe iff the index has codes, ip, no filter, a cut of at most 1024, a batch within the measured limit
    assert codes._use_approx_probe(None, "ip", None, 10, None) is True and no_codes._use_approx_probe(None, "ip", None, 10, None) is False
    assert codes._use_approx_probe(None, "ip", None, 512, None) is True and codes._use_approx_probe(None, "ip", None, 513, None) is False
    assert codes._use_approx_probe(None, "ip", None, 5, 1025) is False
    assert codes._use_approx_probe(None, "ip", object(), 10, None) is False
    assert codes._use_approx_probe(None, "one_minus_dist", None, 10, 10) is False
    assert codes._use_approx_probe(False, "ip", None, 10, None) is False and codes._use_approx_probe(True, "ip", None, 10, None, 999) is True
    cap = IVFIndex.APPROX_AUTO_MAX_BATCH
    assert cap is None or (isinstance(cap, int) and cap >= 1)
    if cap is not None:
        assert codes._use_approx_probe(None, "ip", None, 10, None, cap) is True
        assert codes._use_approx_probe(None, "ip", None, 10, None, cap + 1) is False
    else:
        assert codes._use_approx_probe(None, "ip", None, 10, None, 4096) is True


def test_signatures():
    from dewi._engine import DeviceCorpus, Int8Corpus
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    for name in ("search", "search_batch"):
        params = inspect.signature(getattr(IVFIndex, name)).parameters
        assert list(params)[-1] == "nprobe" and params["nprobe"].kind is inspect.Parameter.KEYWORD_ONLY
        assert params["approx"].default is None and params["rescore"].default is True
    dev = inspect.signature(IVFIndex.search_device).parameters
    assert dev["approx"].default is None and dev["rescore"].default is True and "nprobe" in dev
    assert list(inspect.signature(DeviceCorpus.candidates_i8_filtered_device).parameters) == [
        "self", "q_dev", "n_candidates", "filter", "out", "id_offset"]
    assert list(inspect.signature(DeviceCorpus.search_approx_filtered_device).parameters) == [
        "self", "q_dev", "k", "eta", "entropy_pref", "filter", "candidates", "rescore", "out_ids", "out_scores"]
    assert callable(DeviceCorpus.search_approx_filtered)
    for cls in (ExactIndex, DewiIndex):
        for name, first in (("search_approx_filtered", "query"), ("search_approx_filtered_batch", "queries")):
            ps = inspect.signature(getattr(cls, name)).parameters
            assert list(ps) == ["self", first, "k", "eta", "entropy_pref", "candidates", "filter", "rescore"]
            assert ps["filter"].kind is inspect.Parameter.KEYWORD_ONLY and ps["filter"].default is inspect.Parameter.empty
            assert ps["rescore"].kind is inspect.Parameter.KEYWORD_ONLY and ps["rescore"].default is True
    # a stand-alone int8 corpus has no filters: it keeps refusing everything outside what it serves
    c = object.__new__(Int8Corpus)
    for name in ("make_filter", "make_query_filters", "candidates_i8_filtered_device", "search_approx_filtered_device",
                 "search_approx_filtered"):
        assert name not in Int8Corpus._SERVED
        with pytest.raises(NotImplementedError, match="stand-alone int8 corpus"):
            getattr(c, name)

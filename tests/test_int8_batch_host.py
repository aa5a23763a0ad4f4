"""The int8 batch pass without a GPU: the "supported" predicate and the plan (neither needs a device), the size formula
restated in Python at extreme shapes, and the argument errors of ``dewi_knn_candidates_i8_batch`` — the codes, messages and
precedence of ``dewi_knn_candidates_i8`` (tests/test_int8_host.py), then the shapes the pass itself does not take.  No case
gets as far as the device."""
import ctypes
import inspect

import pytest

OK, INVALID, K_OOB, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -5
ROWS_2_32 = "n_rows 4294967296 exceeds 2^32-1 rows per device"
BIG = 1 << 32
FLOOR, MIN_B, MAX_C = 4096, 2, 256          # csrc/launch.hpp kI8MfmaMinRows, kI8MfmaMinQueries, kMaxListCandidates

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def up(v):
    return (v + 255) // 256 * 256


def model_plan(n, dim, b, c):
    """The plan of csrc/knn_mfma_i8.hip plan_mfma_i8 in Python integers (no 32-bit arithmetic anywhere)."""
    groups = (b + 31) // 32
    q_pad = groups * 32
    n_tiles = (n + 31) // 32
    stride = min(max(4096 // c, 8), 128)
    while stride > 1 and (n_tiles + stride - 1) // stride < 256:
        stride //= 2
    n_sample_tiles = (n_tiles + stride - 1) // stride
    sample_blocks = min(n_sample_tiles, 128)
    n_blocks = min((n_tiles + 7) // 8, 256)
    seg_cap = max(16, (8 * stride * c + n_blocks - 1) // n_blocks)
    slots1 = c <= 64
    steps = (n + 31) // 32
    repair_blocks = min(steps, 256 if slots1 else 64)
    repair_keys = (repair_blocks if slots1 else repair_blocks * 8) * c
    off = 0
    off += up(q_pad * dim)          # query codes
    off += up(q_pad * 4)            # query scales
    off += up(q_pad * 4)            # thresholds
    flags_off = off
    off += up(b * 4)
    cnt_off = off
    off += up(groups * n_blocks * 32 * 4)
    off += up(32 * sample_blocks * 256 * 4)
    cand_off = off
    off += up(groups * n_blocks * 32 * seg_cap * 8)
    total = max(off, cnt_off + up(b * repair_keys * 8))
    fits = n_blocks * 32 * seg_cap < 1 << 32
    return {"groups": groups, "n_blocks": n_blocks, "n_seg": n_blocks, "seg_cap": seg_cap, "tile_stride": stride,
            "n_sample_tiles": n_sample_tiles, "sample_blocks": sample_blocks, "flags_off": flags_off, "cnt_off": cnt_off,
            "cand_off": cand_off, "repair_off": cnt_off, "total": total if fits else 0}


def test_size_is_zero_exactly_for_the_shapes_the_pass_does_not_take(lib):
    size = lib.dewi_knn_i8_batch_workspace_bytes
    for bad in ((FLOOR, 72, 32, 20), (FLOOR, 100, 32, 20),                                   # dim % 16
                (FLOOR, 48, 32, 20), (FLOOR, 16, 32, 20), (FLOOR, 0, 32, 20), (FLOOR, 1552, 32, 20),   # dim < 64, > 1536
                (FLOOR, 768, 32, MAX_C + 1), (FLOOR, 768, 32, 0), (FLOOR, 768, 32, -1),      # the cut
                (FLOOR, 768, MIN_B - 1, 20), (FLOOR, 768, 0, 20), (FLOOR, 768, -3, 20),       # the batch
                (FLOOR, 768, (1 << 20) + 1, 20), (FLOOR, 768, (1 << 31) - 1, 20), (1 << 20, 1536, (1 << 31) - 1, 256),
                (FLOOR - 1, 768, 32, 20), (1, 768, 32, 20), (0, 768, 32, 20), (-5, 768, 32, 20),   # the floor
                (BIG, 768, 32, 20), (BIG + 7, 768, 32, 20)):                                 # 2^32 rows or more
        assert size(*bad) == 0, bad
    from dewi import _native as nat
    with pytest.raises(NotImplementedError, match="the int8 batch pass does not take"):
        nat.i8_batch_plan(FLOOR, 48, 32, 20)
    assert lib.dewi_knn_i8_batch_plan(FLOOR, 768, 32, 20, None) == INVALID


def test_size_is_nonzero_over_the_required_range(lib):
    size = lib.dewi_knn_i8_batch_workspace_bytes
    assert FLOOR <= 16384
    for dim in range(64, 1536 + 1, 16):
        assert size(FLOOR, dim, MIN_B, 1) > 0 and size(1 << 20, dim, 4096, MAX_C) > 0, dim
    for c in (1, 2, 63, 64, 65, 255, 256):
        for b in (MIN_B, 31, 32, 33, 64, 1000, 1 << 20):
            for n in (FLOOR, FLOOR + 37, 16384, 1 << 20, BIG - 1):
                assert size(n, 768, b, c) > 0, (n, b, c)


SHAPES = [(FLOOR, 64, MIN_B, 1), (FLOOR + 37, 768, 32, 20), (3 * FLOOR, 1536, 64, 256), (3 * FLOOR, 272, 33, 65),
          (200_000, 768, 32, 200), (1_000_000, 768, 32, 20), (1_000_000, 768, 256, 200), (1 << 24, 1024, 100, 64),
          (BIG - 1, 1536, 4096, 256), (BIG - 1, 64, MIN_B, 1), (BIG - 1, 1536, 4096, 1)]


@pytest.mark.parametrize("n,dim,b,c", SHAPES)
def test_plan_agrees_with_the_size_and_with_the_formula(lib, n, dim, b, c):
    from dewi import _native as nat
    assert len(nat.I8_BATCH_PLAN_WORDS) == 12
    p = nat.i8_batch_plan(n, dim, b, c)
    want = model_plan(n, dim, b, c)
    assert want["total"] > 0
    assert p == want, (p, want)
    assert p["total"] == lib.dewi_knn_i8_batch_workspace_bytes(n, dim, b, c)
    # ascending, 256-byte aligned, inside the total, room for what lives there
    offs = [p["flags_off"], p["cnt_off"], p["cand_off"]]
    assert offs == sorted(offs) and len(set(offs)) == 3 and all(o % 256 == 0 for o in offs + [p["repair_off"], p["total"]])
    assert p["flags_off"] + 4 * b <= p["cnt_off"]
    assert p["cnt_off"] + 4 * p["groups"] * p["n_seg"] * 32 <= p["cand_off"]
    assert p["cand_off"] + 8 * p["groups"] * p["n_seg"] * 32 * p["seg_cap"] <= p["total"]
    assert p["flags_off"] < p["repair_off"] < p["total"]
    # the plan itself
    assert p["groups"] == (b + 31) // 32 and 1 <= p["n_blocks"] <= 256 and p["n_seg"] == p["n_blocks"] and p["seg_cap"] >= 16
    assert p["n_seg"] * 32 * p["seg_cap"] < 1 << 32
    assert p["sample_blocks"] == min(128, p["n_sample_tiles"]) and p["n_sample_tiles"] * p["tile_stride"] >= (n + 31) // 32
    assert p["n_sample_tiles"] >= min(256, (n + 31) // 32)                 # a sample of a tile per workgroup, or every tile


def test_an_all_ties_query_overflows_its_segments_at_every_size(lib):
    """What tests/test_hip_int8_batch.py relies on to reach the repair: a query every row survives has more survivors than its
    segments hold."""
    from dewi import _native as nat
    for n in (FLOOR, FLOOR + 37, 3 * FLOOR, 65536, 200_000, 1 << 20):
        for c in (1, 20, 64, 65, 256):
            p = nat.i8_batch_plan(n, 768, 32, c)
            assert n > p["n_seg"] * p["seg_cap"], (n, c, p)


def batch(codes=P, scales=P, n=FLOOR, d=768, Q=P, b=32, dewi=P, c=20, id_offset=0, out=P, ws=P, nbytes=1 << 40):
    return lambda lib: lib.dewi_knn_candidates_i8_batch(codes, scales, n, d, Q, b, dewi, P, c, id_offset, out, ws, nbytes, None)


NOT_TAKEN = "the int8 batch pass does not take {} rows x {} columns, {} queries, {} candidates " \
            "(dewi_knn_i8_batch_workspace_bytes is 0: use dewi_knn_candidates_i8)"
CASES = [
    # ---- the errors of dewi_knn_candidates_i8, word for word
    ("null codes", batch(codes=None), INVALID, "null codes, scales or query pointer"),
    ("null scales", batch(scales=None), INVALID, "null codes, scales or query pointer"),
    ("null Q", batch(Q=None), INVALID, "null codes, scales or query pointer"),
    ("n_rows", batch(n=0), INVALID, "n_rows must be positive (got 0)"),
    ("rows", batch(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("dim 0", batch(d=0), INVALID, "dim must be positive (got 0)"),
    ("dim % 16", batch(d=8), UNSUPPORTED, "dim 8: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("dim > 4096", batch(d=8192), UNSUPPORTED, "dim 8192: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("n_queries", batch(b=0), INVALID, "n_queries must be positive (got 0)"),
    ("c <= 0", batch(c=0), INVALID, "n_candidates must be positive (got 0)"),
    ("c > 1024", batch(n=5000, c=1025), UNSUPPORTED, "n_candidates 1025 exceeds the 1024 the int8 route takes"),
    ("null payload", batch(dewi=None), INVALID, "null payload or output pointer"),
    ("null out", batch(out=None), INVALID, "null payload or output pointer"),
    ("alignment of the codes", batch(codes=P + 4), INVALID, "the codes must be 16-byte aligned"),
    ("alignment of the queries", batch(Q=P + 8), INVALID, "the queries must be 16-byte aligned"),
    ("id_offset", batch(id_offset=-1), UNSUPPORTED, f"global row ids must fit int32 (offset -1 + {FLOOR} rows)"),
    ("id range", batch(id_offset=(1 << 31) - FLOOR), UNSUPPORTED,
     f"global row ids must fit int32 (offset {(1 << 31) - FLOOR} + {FLOOR} rows)"),
    ("order: null before the shape", batch(codes=None, d=24), INVALID, "null codes, scales or query pointer"),
    ("order: the shape before the cut", batch(d=24, c=2000), UNSUPPORTED,
     "dim 24: the int8 route takes dim % 16 == 0 up to 4096 columns"),
    ("order: n_queries before the cut", batch(b=-1, c=2000), INVALID, "n_queries must be positive (got -1)"),
    ("order: the cut before the null payload", batch(c=2000, dewi=None), UNSUPPORTED,
     "n_candidates 2000 exceeds the 1024 the int8 route takes"),
    ("order: the null payload before the alignment", batch(out=None, codes=P + 4), INVALID, "null payload or output pointer"),
    ("order: the alignment before the id range", batch(codes=P + 4, id_offset=-1), INVALID, "the codes must be 16-byte aligned"),
    # ---- then what the pass itself does not take, before the workspace
    ("pass: dim 48", batch(d=48), UNSUPPORTED, NOT_TAKEN.format(FLOOR, 48, 32, 20)),
    ("pass: dim 2048", batch(d=2048), UNSUPPORTED, NOT_TAKEN.format(FLOOR, 2048, 32, 20)),
    ("pass: c 300", batch(c=300), UNSUPPORTED, NOT_TAKEN.format(FLOOR, 768, 32, 300)),
    ("pass: one query", batch(b=1), UNSUPPORTED, NOT_TAKEN.format(FLOOR, 768, 1, 20)),
    ("pass: below the floor", batch(n=FLOOR - 1), UNSUPPORTED, NOT_TAKEN.format(FLOOR - 1, 768, 32, 20)),
    ("order: the id range before the pass's shape", batch(d=48, id_offset=-1), UNSUPPORTED,
     f"global row ids must fit int32 (offset -1 + {FLOOR} rows)"),
    ("order: the pass's shape before the workspace", batch(b=1, nbytes=16), UNSUPPORTED, NOT_TAKEN.format(FLOOR, 768, 1, 20)),
    # ---- the workspace
    ("workspace", batch(nbytes=16), WORKSPACE, None),
    ("null workspace", batch(ws=None), WORKSPACE, None),
    ("workspace alignment", batch(ws=P + 4), INVALID, "the workspace must be 16-byte aligned"),
]


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


def test_a_short_workspace_names_the_required_size(lib):
    from dewi import _native as nat
    need = lib.dewi_knn_i8_batch_workspace_bytes(FLOOR, 768, 32, 20)
    assert batch(nbytes=need - 1)(lib) == WORKSPACE
    assert nat.last_error() == f"workspace {need - 1} B < required {need} B"


def test_the_row_entry_point_keeps_its_size_and_codes(lib):
    """``dewi_knn_candidates_i8`` is unchanged: the same workspace size, and the batch shapes it always took are no error."""
    assert lib.dewi_knn_i8_workspace_bytes(1 << 20, 768, 32, 20) == 32 * 256 * 20 * 8
    rc = lib.dewi_knn_candidates_i8(P, P, 1 << 20, 768, P, 32, P, P, 20, 0, P, P, 16, None)
    assert rc == WORKSPACE


def test_python_signatures():
    from dewi._engine import DeviceCorpus, Int8Corpus
    for fn in (DeviceCorpus.candidates_i8_device, DeviceCorpus.search_approx, Int8Corpus.search_approx):
        assert inspect.signature(fn).parameters["batch_pass"].default is None, fn

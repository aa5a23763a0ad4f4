"""In-place removal / upsert, the host side (no GPU): ``plan_remove`` against the model of tests/mutate_model.py, its
validation, the argument errors of the two new exports through ctypes (a call that fails here has enqueued nothing), the
symbols in header / ``EXPORTED_SYMBOLS`` / library / INTEGRATION.md, and ``PayloadStore.follow`` on host columns."""
import ctypes
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import mutate_model as mm

REPO = Path(__file__).resolve().parent.parent
NEW_EXPORTS = {"dewi_rows_move", "dewi_rows_put_f32"}
OK, INVALID, UNSUPPORTED = 0, -1, -5
BIG = 1 << 32

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer


# ------------------------------------------------------------------------------------------------ plan_remove
def _check_plan(n, deleted):
    from dewi._engine import plan_remove
    src, dst, n_keep = plan_remove(n, np.asarray(deleted, dtype=np.int64))
    movers, holes, keep = mm.remove_pairs(n, deleted)
    assert src.dtype == np.int64 and dst.dtype == np.int64
    assert (src.tolist(), dst.tolist(), n_keep) == (movers, holes, keep), (n, sorted(deleted))


def test_plan_remove_equals_the_model_for_every_subset_up_to_8_rows():
    cases = 0
    for n in range(1, 9):
        for m in range(0, n):                          # (all n rows: refused, below)
            for dele in itertools.combinations(range(n), m):
                _check_plan(n, list(dele))
                cases += 1
    assert cases == sum(2 ** n - 1 for n in range(1, 9))


def test_plan_remove_equals_the_model_on_random_cases():
    rs = np.random.RandomState(7)
    for case in range(200):
        n = int(rs.randint(1, 5001))
        m = int(rs.randint(0, n)) if case % 4 else int(rs.randint(n // 2, n))     # every fourth: more than half
        _check_plan(n, rs.permutation(n)[:m].tolist())                             # (in no particular order)


def test_plan_remove_takes_any_integer_dtype_and_order():
    from dewi._engine import plan_remove
    src, dst, n_keep = plan_remove(6, np.array([4, 1], dtype=np.int32))
    assert (src.tolist(), dst.tolist(), n_keep) == ([5], [1], 4)
    src, dst, n_keep = plan_remove(6, [])
    assert (src.size, dst.size, n_keep) == (0, 0, 6)


@pytest.mark.parametrize("n,rows,message", [
    (5, [0.5], "rows to remove must be integers"),
    (5, [5], r"rows to remove must lie in \[0, 5\)"),
    (5, [-1], r"rows to remove must lie in \[0, 5\)"),
    (5, [1, 3, 1], "rows to remove must be distinct"),
    (3, [0, 1, 2], "cannot remove every row"),
    (1, [0], "cannot remove every row"),
])
def test_plan_remove_validation(n, rows, message):
    from dewi._engine import plan_remove
    with pytest.raises(ValueError, match=message):
        plan_remove(n, np.asarray(rows))


# ------------------------------------------------------------------------------------------------ the two exports
def move(E=P, elem=0, shadow=P, dewi=P, ent=P, aux=P, n=10, d=8, keep=8, src=P, dst=P, moves=2, err=P):
    return lambda lib: lib.dewi_rows_move(E, elem, shadow, dewi, ent, aux, n, d, keep, src, dst, moves, err, None)


def put(E=P, shadow=P, dewi32=P, ent=P, cap=10, d=8, norm=1, raw=P, dewi=P, ht=P, hi=P, rows=P, m=2, err=P):
    return lambda lib: lib.dewi_rows_put_f32(E, shadow, dewi32, ent, cap, d, norm, raw, dewi, ht, hi, rows, m, err, None)


CASES = [
    ("move null matrix", move(E=None), INVALID, "null pointer"),
    ("move null payload", move(ent=None), INVALID, "null pointer"),
    ("move null pairs", move(dst=None), INVALID, "null pointer"),
    ("move null error word", move(err=None), INVALID, "null pointer"),
    ("move dim", move(d=0), INVALID, "dim must be positive (got 0)"),
    ("move elem_type", move(elem=2), INVALID, "unknown elem_type 2"),
    ("move negative", move(moves=-1), INVALID, "negative count (n_rows 10, n_keep 8, n_moves -1)"),
    ("move n_keep > n_rows", move(keep=11), INVALID, "n_keep 11 exceeds n_rows 10"),
    ("move rows", move(n=BIG, keep=BIG - 2), UNSUPPORTED, "n_rows 4294967296 exceeds 2^32-1 rows per device"),
    ("move shadow of a bf16 matrix", move(elem=1), INVALID, "a bf16 main matrix takes no bf16 shadow"),
    ("move bf16 matrix without a shadow: no moves", move(elem=1, shadow=None, moves=0), OK, None),
    ("move more moves than tail rows", move(moves=3), INVALID, "n_moves 3 exceeds the 2 rows above n_keep or the 8 below it"),
    ("move nothing", move(moves=0, E=None, src=None, dst=None), OK, None),
    ("move order: dim before the counts", move(d=-1, keep=11), INVALID, "dim must be positive (got -1)"),
    ("put null matrix", put(E=None), INVALID, "null pointer"),
    ("put null staging", put(raw=None), INVALID, "null pointer"),
    ("put null triple", put(hi=None), INVALID, "null pointer"),
    ("put null slots", put(rows=None), INVALID, "null pointer"),
    ("put null error word", put(err=None), INVALID, "null pointer"),
    ("put dim", put(d=0), INVALID, "dim must be positive (got 0)"),
    ("put negative", put(m=-2), INVALID, "negative count (capacity_rows 10, n_put -2)"),
    ("put capacity", put(cap=BIG), UNSUPPORTED, "capacity_rows 4294967296 exceeds 2^32-1 rows per device"),
    ("put more rows than capacity", put(m=11), INVALID, "n_put 11 exceeds capacity_rows 10"),
    ("put nothing", put(m=0, raw=None, rows=None), OK, None),
    ("put order: dim before the counts", put(d=0, m=-1), INVALID, "dim must be positive (got 0)"),
]


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_case_names_are_unique():
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("name,call,code,message", CASES, ids=[c[0] for c in CASES])
def test_argument_error(lib, name, call, code, message):
    from dewi import _native as nat
    rc = call(lib)
    got = nat.last_error()
    print(f"{name}: rc {rc}, {got!r}")
    assert rc == code, (name, rc, got)
    if message is not None:
        assert got == message, name


def test_the_symbols_are_declared_exported_and_documented(lib):
    from dewi import _native as nat
    header = (REPO / "include" / "dewi_hip.h").read_text()
    declared = set(re.findall(r"\b(dewi_[a-z0-9_]+)\s*\(", header))
    assert NEW_EXPORTS <= declared
    assert NEW_EXPORTS <= set(nat.EXPORTED_SYMBOLS)
    assert set(nat.EXPORTED_SYMBOLS) == declared
    for name in NEW_EXPORTS:
        assert hasattr(lib, name)
        assert f"`{name}`" in (REPO / "INTEGRATION.md").read_text()
    assert "no counterpart" in header[header.index("In-place mutation"):header.index("int dewi_rows_move")]
    assert lib.dewi_abi_version() == 6 and "#define DEWI_ABI_VERSION 6" in header
    assert "mutate.hip" in (REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd" / "csrc" / "Makefile").read_text()


# ------------------------------------------------------------------------------------------------ PayloadStore.follow
def _store():
    """Rows 0-2 objects, rows 3-7 one column block, row 8 an object."""
    from dewi.types import Payload, PayloadStore
    s = PayloadStore()
    ids = [f"d{i}" for i in range(9)]
    objs = {i: Payload(dewi=float(i), ht_mean=10.0 + i) for i in (0, 1, 2, 8)}
    for i, p in objs.items():
        s[ids[i]] = p
    s.add_columns(3, ids[3:8], {"dewi": np.arange(3, 8, dtype=np.float64), "hi_mean": 100.0 + np.arange(3, 8)})
    return s, ids, objs


def _columns(store, ids):
    """(dewi, ht_mean, hi_mean) per row as ExactIndex._payload_columns reads them: blocks, made objects, then dict objects."""
    n = len(ids)
    out = np.full((3, n), np.nan)
    for row0, row1, cols, made in store.column_blocks():
        for f, name in enumerate(("dewi", "ht_mean", "hi_mean")):
            out[f, row0:row1] = cols.get(name, np.zeros(row1 - row0))
        for row, p in made.items():
            out[:, row] = (p.dewi, p.ht_mean, p.hi_mean)
    for r in np.flatnonzero(np.isnan(out[0])).tolist():
        p = dict.__getitem__(store, ids[r])
        out[:, r] = (p.dewi, p.ht_mean, p.hi_mean)
    return out


def test_payload_store_follows_a_removal():
    s, ids, objs = _store()
    handed_out = s["d5"]                                   # a column row's object, made on demand
    before = _columns(s, ids)
    dele = ["d1", "d4", "d8"]
    order = mm.remove_order(9, [1, 4, 8])                  # [0, 7, 2, 3, 6, 5]
    new_ids = [ids[i] for i in order.tolist()]
    s.follow(order, 9, new_ids, removed=dele)
    assert len(s) == 6 and all(d not in s for d in dele) and s.get("d4") is None
    assert s["d5"] is handed_out and s["d0"] is objs[0] and s["d2"] is objs[2]
    assert np.array_equal(_columns(s, new_ids), before[:, order])
    for r, d in enumerate(new_ids):
        assert s.at_row(r, d) is s[d]
    assert (s["d7"].dewi, s["d7"].hi_mean, s["d7"].ht_mean) == (7.0, 107.0, 0.0)
    assert sorted(s.keys()) == sorted(new_ids)


def test_payload_store_follows_upserts_as_objects_and_as_columns():
    from dewi.types import Payload
    s, ids, objs = _store()
    old = s["d6"]
    # objects: d6 (a column row) replaced, x appended
    p6, px = Payload(dewi=-6.0), Payload(dewi=-1.0, hi_mean=5.0)
    ids2 = ids + ["x"]
    order = np.array([0, 1, 2, 3, 4, 5, -1, 7, 8, -1])
    s.follow(order, 9, ids2, objects=[(6, "d6", p6), (9, "x", px)])
    assert s["d6"] is p6 and s["d6"] is not old and s["x"] is px and len(s) == 10
    cols = _columns(s, ids2)
    assert cols[0].tolist() == [0, 1, 2, 3, 4, 5, -6, 7, 8, -1] and cols[2, 9] == 5.0 and cols[2, 6] == 0.0
    # columns: d0 (an object row) replaced, y appended; the old object of d0 is dropped
    ids3 = ids2 + ["y"]
    order = np.array([-1, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1])
    s.follow(order, 10, ids3, columns=(np.array([0, 10]), ["d0", "y"], {"dewi": np.array([50.0, 60.0]), "ht_mean": np.array([1.0, 2.0])}))
    assert s["d0"] is not objs[0] and (s["d0"].dewi, s["d0"].ht_mean) == (50.0, 1.0) and s["y"].dewi == 60.0
    assert s["d6"] is p6 and s["d1"] is objs[1] and len(s) == 11
    cols = _columns(s, ids3)
    assert cols[0].tolist() == [50, 1, 2, 3, 4, 5, -6, 7, 8, -1, 60]
    assert cols[1].tolist() == [1, 11, 12, 0, 0, 0, 0, 0, 18, 0, 2]


def test_a_store_of_objects_only_stays_a_plain_dict():
    from dewi.types import Payload, PayloadStore
    s = PayloadStore()
    ps = [Payload(dewi=float(i)) for i in range(4)]
    for i, p in enumerate(ps):
        s[f"d{i}"] = p
    s.follow(mm.remove_order(4, [1]), 4, ["d0", "d3", "d2"], removed=["d1"])
    assert not s._blocks and len(s) == 3 and s["d3"] is ps[3] and "d1" not in s


def test_later_mutations_are_applied_in_place_and_equal_the_re_gather():
    """``follow_remove`` / ``follow_put`` on the store's own block (after a first ``follow``) against the general path on a
    twin store, step by step: columns, ids, objects, length."""
    from dewi.types import Payload

    def twin():
        s, ids, _ = _store()
        s["d5"], s["d7"]                                   # two column rows get their objects
        return s, list(ids)

    (a, ids_a), (b, ids_b) = twin(), twin()
    rs = np.random.RandomState(0)
    fresh = 0
    for step in range(12):
        n = len(ids_a)
        if step % 3 == 0 and n > 3:                        # remove 1-3 documents
            rows = rs.choice(n, int(rs.randint(1, 4)), replace=False)
            gone = [ids_a[r] for r in rows.tolist()]
            movers, holes, n_keep = mm.remove_pairs(n, rows.tolist())
            order = mm.remove_order(n, rows.tolist())
            new_ids = [ids_a[i] for i in order.tolist()]
            a.follow_remove(np.array(movers, dtype=np.int64), np.array(holes, dtype=np.int64), n, new_ids, gone, rows)
            b._owned = False
            b.follow(order, n, new_ids, removed=gone)
        else:                                              # upsert one known and one new document, as objects or as columns
            known = ids_a[int(rs.randint(0, n))]
            ups = [f"n{fresh}", known]
            fresh += 1
            rows_l, new_ids = mm.upsert_rows(ids_a, ups)
            rows = np.array(rows_l, dtype=np.int64)
            order = np.concatenate([np.arange(n), [-1]])
            order[rows] = -1
            if step % 3 == 1:
                ps = [Payload(dewi=100.0 + step, hi_mean=1.0), Payload(dewi=200.0 + step, ht_mean=2.0)]
                a.follow_put(rows, n, new_ids, ups, objects=ps)
                b._owned = False
                b.follow(order, n, new_ids, objects=list(zip(rows_l, ups, ps)))
            else:
                cols = {"dewi": np.array([300.0 + step, 400.0 + step]), "ht_mean": np.array([3.0, 4.0])}
                a.follow_put(rows, n, new_ids, ups, columns=cols)
                b._owned = False
                b.follow(order, n, new_ids, columns=(rows, ups, cols))
        ids_a = ids_b = new_ids
        if step:
            assert a._owned and len(a._blocks) == 1
        assert list(a._blocks[0][2]) == new_ids == list(b._blocks[0][2]) and a._blocks[0][:2] == (0, len(new_ids))
        assert np.array_equal(_columns(a, new_ids), _columns(b, new_ids)), step
        assert len(a) == len(b) == len(new_ids) and sorted(a._made[0]) == sorted(b._made[0])
        for r, d in enumerate(new_ids):
            pa, pb = a.at_row(r, d), b.at_row(r, d)
            assert pa == pb and pa is a[d], (step, d)

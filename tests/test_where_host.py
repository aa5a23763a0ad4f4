"""Predicates over attribute columns, the host half (no GPU): the NumPy model against a per-row stack machine, the
expression compiler of ``dewi.where``, the column encoder and the files of ``dewi.attributes``, and every argument error of
``dewi_predicate_masks`` by code and text in the order include/dewi_hip.h states (the library loads without a GPU and these
errors come before the first device call, as in ``test_abi_errors_host.py``).
"""
import ctypes
import json
import math
import struct

import numpy as np
import pytest

import predicate_model as pm
from predicate_model import OP

OK, INVALID, UNSUPPORTED = 0, -1, -5
SCHEMA = {"year": ("int", None), "tags": ("int", None), "noise": ("float", None), "site": ("cat", ["a.org", "b.org", "c.org"])}


# ---------------------------------------------------------------------------------------------- the model
def evaluate_naive(columns, types, program, sets, base=None):
    """The contract of include/dewi_hip.h one row at a time, in plain Python: a stack of bits per row."""
    n = len(columns[0])
    out = np.zeros(n, dtype=np.uint8)
    for r in range(n):
        st = []
        for op, c, a, b in program:
            name = pm.OPS[op]
            if name == "AND":
                y = st.pop(); st[-1] = st[-1] and y
            elif name == "OR":
                y = st.pop(); st[-1] = st[-1] or y
            elif name == "NOT":
                st[-1] = not st[-1]
            elif name == "TRUE":
                st.append(True)
            elif name.startswith("I_"):
                u = int(np.asarray(columns[c][r]).view(np.uint32))
                x = u - (1 << 32) if u >= (1 << 31) else u
                ia = a - (1 << 32) if a >= (1 << 31) else a
                ib = b - (1 << 32) if b >= (1 << 31) else b
                if name == "I_IN_SET":
                    st.append(0 <= x < b and bool((int(sets[a + x // 32]) >> (x % 32)) & 1))
                else:
                    st.append({"I_LT": x < ia, "I_LE": x <= ia, "I_EQ": x == ia, "I_NE": x != ia, "I_GE": x >= ia, "I_GT": x > ia,
                               "I_BETWEEN": ia <= x <= ib, "I_ANY_BITS": (u & a) != 0, "I_ALL_BITS": (u & a) == a}[name])
            else:
                f = float(columns[c][r])
                fa = struct.unpack("<f", struct.pack("<I", a))[0]
                fb = struct.unpack("<f", struct.pack("<I", b))[0]
                st.append({"F_LT": f < fa, "F_LE": f <= fa, "F_EQ": f == fa, "F_NE": f != fa, "F_GE": f >= fa, "F_GT": f > fa,
                           "F_BETWEEN": fa <= f <= fb, "F_IS_NAN": math.isnan(f)}[name])
        assert len(st) == 1
        out[r] = 1 if st[0] and (base is None or base[r] != 0) else 0
    return out


def test_model_equals_the_per_row_stack_machine():
    rs = np.random.RandomState(5)
    n = 97
    types = [0, 1, 0, 1]
    cols = [pm.edge_column(rs, n, t) for t in types]
    cols[0][:len(pm.INT_EDGES)] = pm.INT_EDGES
    cols[1][:len(pm.FLOAT_EDGES)] = pm.FLOAT_EDGES
    sets, table = pm.random_sets(rs)
    base = (rs.rand(n) < 0.7).astype(np.uint8) * 3
    depths = []
    for i in range(60):
        prog = pm.random_program(rs, types, table, length=1 + (i * 7) % 64)
        from dewi.where import program_depth
        depths.append(program_depth(prog))
        for b in (None, base):
            got = pm.evaluate(cols, types, prog, sets, b)
            assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
            assert np.array_equal(got, evaluate_naive(cols, types, prog, sets, b)), prog
    assert max(depths) >= 16 and min(depths) == 1           # the generator reaches deep stacks as well as single leaves


def test_random_programs_reach_the_limits():
    from dewi.where import program_depth
    rs = np.random.RandomState(1)
    deep = [program_depth(pm.random_program(rs, [0, 1], (), length=64)) for _ in range(200)]
    assert max(deep) == 32
    for length in (1, 2, 3, 63, 64):
        assert len(pm.random_program(rs, [0], (), length=length)) == length


def test_ieee_rules_of_the_float_leaves():
    x = np.array([np.nan, 0.0, -0.0, 1.0, np.inf], dtype=np.float32)
    zero = 0
    neg_zero = 0x80000000
    nan = 0x7FC00000

    def run(op, a, b=0):
        return pm.evaluate([x], [1], [(OP[op], 0, a, b)], []).tolist()
    assert run("F_EQ", zero) == [0, 1, 1, 0, 0] == run("F_EQ", neg_zero)     # -0 equals +0
    assert run("F_NE", zero) == [1, 0, 0, 1, 1]                              # NaN != c is true
    for op in ("F_LT", "F_LE", "F_GE", "F_GT", "F_EQ"):
        assert run(op, zero)[0] == 0 and run(op, nan) == [0] * 5             # every other compare with a NaN is false
    assert run("F_NE", nan) == [1] * 5
    assert run("F_BETWEEN", neg_zero, 0x3F800000) == [0, 1, 1, 1, 0]
    assert run("F_IS_NAN", 0) == [1, 0, 0, 0, 0]


def test_in_set_reads_no_word_outside_the_set():
    x = np.array([-1, 0, 4, 5, 31, 32, (1 << 31) - 1, -(1 << 31)], dtype=np.int32)
    sets = np.array([0xFFFFFFFF, 0b10001, 0xFFFFFFFF], dtype=np.uint32)      # a 5-bit set at word 1 between poison words
    got = pm.evaluate([x], [0], [(OP["I_IN_SET"], 0, 1, 5)], sets)
    assert got.tolist() == [0, 1, 1, 0, 0, 0, 0, 0]                          # x == b and beyond: false, whatever the words hold


# ---------------------------------------------------------------------------------------------- expressions -> programs
def prog(where, schema=SCHEMA):
    from dewi.where import compile_programs
    p = compile_programs([where], schema)
    return p.columns, [(pm.OPS[op], c, a, b) for op, c, a, b in p.programs[0]], p.sets


def f32_bits(v):
    return int(np.asarray(np.float32(v)).view(np.uint32))


def test_every_operator_compiles_to_its_op():
    from dewi.where import col
    y, t, z, s = col("year"), col("tags"), col("noise"), col("site")
    for where, op in ((y < 5, "I_LT"), (y <= 5, "I_LE"), (y == 5, "I_EQ"), (y != 5, "I_NE"), (y >= 5, "I_GE"), (y > 5, "I_GT")):
        cols, p, sets = prog(where)
        assert cols == ["year"] and p == [(op, 0, 5, 0)] and sets.size == 0
    assert prog(y > -1)[1] == [("I_GT", 0, 0xFFFFFFFF, 0)]
    assert prog(y.between(-2, 7))[1] == [("I_BETWEEN", 0, 0xFFFFFFFE, 7)]
    assert prog(t.any_bits(0b1010))[1] == [("I_ANY_BITS", 0, 10, 0)]
    assert prog(t.all_bits(0x80000001))[1] == [("I_ALL_BITS", 0, 0x80000001, 0)]
    assert prog(y == True)[1] == [("I_EQ", 0, 1, 0)]                          # noqa: E712  (bools are integers)
    for where, op in ((z < .5, "F_LT"), (z <= .5, "F_LE"), (z == .5, "F_EQ"), (z != .5, "F_NE"), (z >= .5, "F_GE"), (z > .5, "F_GT")):
        assert prog(where)[1] == [(op, 0, f32_bits(.5), 0)]
    assert prog(z.between(0, 1))[1] == [("F_BETWEEN", 0, 0, f32_bits(1.0))]   # an integer constant is a number for a float column
    assert prog(z.isnan())[1] == [("F_IS_NAN", 0, 0, 0)]
    assert prog(s == "b.org")[1] == [("I_EQ", 0, 1, 0)]
    assert prog(s != "c.org")[1] == [("I_NE", 0, 2, 0)]


def test_isin_is_a_bitset_in_every_case():
    from dewi.where import col
    cols, p, sets = prog(col("year").isin([3, 7, 40]))
    assert p == [("I_IN_SET", 0, 0, 41)] and sets.dtype == np.uint32
    assert sets.tolist() == [(1 << 3) | (1 << 7), 1 << 8]
    assert prog(col("year").isin([2]))[1] == [("I_IN_SET", 0, 0, 3)]          # one value: still a set, no compare
    assert prog(col("year").isin([]))[1] == [("I_IN_SET", 0, 0, 0)]           # the empty set matches nothing
    # two sets in one program lie behind each other
    cols, p, sets = prog(col("year").isin([1, 33]) | col("tags").isin([0]))
    assert p == [("I_IN_SET", 0, 0, 34), ("I_IN_SET", 1, 2, 1), ("OR", 0, 0, 0)] and sets.tolist() == [2, 2, 1]
    for bad in ([-1], [1 << 24], [0, 1 << 30]):
        with pytest.raises(ValueError, match="isin values must lie in"):
            prog(col("year").isin(bad))
    assert prog(col("year").isin([(1 << 24) - 1]))[1] == [("I_IN_SET", 0, 0, 1 << 24)]


def test_precedence_and_negation():
    from dewi.where import col
    a, b, c = col("year") > 1, col("noise") < 2, col("tags") == 3
    la, lb, lc = ("I_GT", 0, 1, 0), ("F_LT", 1, f32_bits(2), 0), ("I_EQ", 2, 3, 0)
    AND, OR, NOT = ("AND", 0, 0, 0), ("OR", 0, 0, 0), ("NOT", 0, 0, 0)
    assert prog(a & b | c)[1] == [la, lb, AND, lc, OR]                        # & binds tighter than |
    assert prog(a | (col("noise") < 2) & (col("tags") == 3))[1] == [la, lb, lc, AND, OR]
    assert prog((a | b) & c)[1] == [la, lb, OR, lc, AND]
    assert prog(~a & b)[1] == [la, NOT, lb, AND]                              # ~ binds tightest
    assert prog(~(a & b))[1] == [la, lb, AND, NOT]
    assert prog(~~a)[1] == [la, NOT, NOT]
    # the column table is in order of first use and shared by the programs of one call
    from dewi.where import compile_programs
    p = compile_programs([b, a & b], SCHEMA)
    assert p.columns == ["noise", "year"] and [i[1] for i in p.programs[1] if i[0] < OP["TRUE"]] == [1, 0]
    with pytest.raises(TypeError, match="no truth value"):
        bool(a)
    with pytest.raises(TypeError, match="parenthesise"):
        a & 3


def test_vocabulary_unknown_string_and_none():
    from dewi.where import col
    s = col("site")
    assert prog(s == "nowhere.org")[1] == [("I_EQ", 0, 3, 0)]                 # a code no row holds (codes are -1 .. 2)
    assert prog(s != "nowhere.org")[1] == [("I_NE", 0, 3, 0)]
    assert prog(s == None)[1] == [("I_EQ", 0, 0xFFFFFFFF, 0)]                 # noqa: E711  (None is the code -1)
    cols, p, sets = prog(s.isin(["c.org", "nowhere.org", "a.org"]))
    assert p == [("I_IN_SET", 0, 0, 3)] and sets.tolist() == [0b101]          # unknown strings drop out of the set
    cols, p, sets = prog(s.isin(["b.org", None]))
    assert p == [("I_IN_SET", 0, 0, 2), ("I_EQ", 0, 0xFFFFFFFF, 0), ("OR", 0, 0, 0)]
    assert prog(s.isin(["nowhere.org"]))[1] == [("I_IN_SET", 0, 0, 0)]
    # the model agrees: an unknown string matches nothing, != matches everything
    codes = np.array([-1, 0, 1, 2], dtype=np.int32)
    for where, want in ((s == "nowhere.org", [0, 0, 0, 0]), (s != "nowhere.org", [1, 1, 1, 1]), (s.isin(["b.org", None]), [1, 0, 1, 0])):
        from dewi.where import compile_programs
        c = compile_programs([where], SCHEMA)
        assert pm.evaluate([codes], [0], c.programs[0], c.sets).tolist() == want


def test_float_constants_are_rounded_to_fp32_once():
    from dewi.where import col
    z = col("noise")
    assert prog(z < 0.1)[1] == [("F_LT", 0, f32_bits(0.1), 0)]
    assert f32_bits(0.1) == 0x3DCCCCCD                                       # fp32(0.1), above the float64 0.1
    # fp32(x) op fp32(c): the fp32 nearest to 0.1 is NOT below the float64 constant 0.1, and it is not below fp32(0.1)
    x = np.array([np.float32(0.1)], dtype=np.float32)
    assert float(x[0]) > 0.1 and pm.evaluate([x], [1], [(OP["F_LT"], 0, f32_bits(0.1), 0)], []).tolist() == [0]
    assert prog(z > 1e40)[1] == [("F_GT", 0, 0x7F800000, 0)]                  # beyond fp32: +inf
    assert prog(z == float("nan"))[1][0][2] & 0x7FC00000 == 0x7FC00000
    assert prog(z >= np.float64(1) / 3)[1] == [("F_GE", 0, f32_bits(np.float32(1 / 3)), 0)]
    import dewi.where as where_module
    assert "fp32(x) op fp32(c)" in where_module.__doc__


def test_compile_errors_are_value_errors():
    from dewi.where import col, compile_programs
    y, z, s = col("year"), col("noise"), col("site")
    cases = [
        (col("nope") > 1, "unknown attribute column 'nope'"),
        (y == "a.org", "not categorical"),
        (z == "a.org", "not categorical"),
        (y.isin(["a.org"]), "not categorical"),
        (y > 2020.5, "an int column takes integer constants"),
        (y.between(1, 2.0), "an int column takes integer constants"),
        (y.isnan(), "is a float operator"),
        (z.any_bits(3), "is an integer operator"),
        (z.all_bits(3), "is an integer operator"),
        (z.isin([1, 2]), "is an integer operator"),
        (y > (1 << 31), "outside int32"),
        (y < -(1 << 31) - 1, "outside int32"),
        (col("tags").any_bits(1 << 32), "outside 32 bits"),
        (s < "b.org", "takes ==, != and isin"),
        (s == 3, "compared with strings or None"),
        (z < None, "takes numbers"),
    ]
    for where, text in cases:
        with pytest.raises(ValueError, match=text):
            compile_programs([where], SCHEMA)
    # over the limits: 33 leaves and 32 ANDs are 65 instructions; a right-nested chain of 33 leaves is 33 deep
    leaf = y > 0
    w = leaf
    for _ in range(32):
        w = w & leaf
    with pytest.raises(ValueError, match="65 instructions"):
        compile_programs([w], SCHEMA)
    w = leaf
    for _ in range(31):
        w = w & leaf
    assert len(compile_programs([w], SCHEMA).programs[0]) == 63
    deep = leaf
    for _ in range(31):
        deep = leaf & deep                                                    # leaf leaf ... AND AND: 32 deep, 63 long
    from dewi.where import program_depth
    assert program_depth(compile_programs([deep], SCHEMA).programs[0]) == 32
    with pytest.raises(ValueError, match="65 instructions"):                  # (33 deep takes 33 pushes and 32 folds: 65)
        compile_programs([leaf & deep], SCHEMA)
    with pytest.raises(ValueError, match="1 .. 256 predicates"):
        compile_programs([leaf] * 257, SCHEMA)
    with pytest.raises(ValueError, match="1 .. 256 predicates"):
        compile_programs([], SCHEMA)
    wide = {f"c{i}": ("int", None) for i in range(17)}
    with pytest.raises(ValueError, match="more than 16 columns"):
        compile_programs([col(f"c{i}") > 0 for i in range(17)], wide)


def test_depth_limit_alone():
    """A valid program of 64 instructions is at most 32 deep (33 pushes need 32 folds): ``program_depth`` is held to
    hand-made programs on both sides of the limit, and the compiler to a 32-deep chain of ``always()``."""
    from dewi.where import always, compile_programs, program_depth
    t, a = (OP["TRUE"], 0, 0, 0), (OP["AND"], 0, 0, 0)
    assert program_depth([t] * 32 + [a] * 31) == 32
    assert program_depth([t] * 33 + [a] * 32) == 33
    with pytest.raises(ValueError, match="pops an empty stack"):
        program_depth([t, a])
    with pytest.raises(ValueError, match="ends with 2 values"):
        program_depth([t, t])
    w = always()
    for _ in range(31):
        w = always() & w
    assert program_depth(compile_programs([w], {}).programs[0]) == 32


# ---------------------------------------------------------------------------------------------- columns and files
def test_encode_column_kinds_and_errors():
    from dewi.attributes import encode_column, fill_value
    kind, v, vocab = encode_column([1, 2, 3], "a")
    assert (kind, v.dtype, vocab) == ("int", np.int32, None)
    kind, v, _ = encode_column(np.array([True, False]), "a")
    assert kind == "int" and v.tolist() == [1, 0]
    kind, v, _ = encode_column(np.array([0.1, 2.0], dtype=np.float64), "a")
    assert kind == "float" and v.dtype == np.float32 and v[0] == np.float32(0.1)          # rounded once
    kind, v, vocab = encode_column(["b", None, "a", "b"], "a")
    assert (kind, v.tolist(), vocab) == ("cat", [1, -1, 0, 1], ["a", "b"])                  # sorted unique; None is -1
    assert encode_column(np.array([(1 << 31) - 1, -(1 << 31)], dtype=np.int64), "a")[1].tolist() == [(1 << 31) - 1, -(1 << 31)]
    for bad in ([1 << 31], [-(1 << 31) - 1], np.array([1 << 40], dtype=np.uint64)):
        with pytest.raises(ValueError, match="do not fit int32"):
            encode_column(bad, "a")
    with pytest.raises(ValueError, match="holds strings or None"):
        encode_column(["a", 3], "a")
    with pytest.raises(ValueError, match="holds numbers"):
        encode_column(["a"], "a", kind="int")
    with pytest.raises(ValueError, match="is categorical"):
        encode_column([1], "a", kind="cat")
    with pytest.raises(ValueError, match="holds integers, got floats"):
        encode_column([1.5], "a", kind="int")
    assert encode_column([1, 2], "a", kind="float")[1].dtype == np.float32
    assert fill_value("int") == 0 and math.isnan(fill_value("float")) and fill_value("cat") == -1


def test_set_attributes_argument_errors_come_before_any_device_work():
    """An index that was never built (and cannot be, without a GPU) still refuses bad columns."""
    from dewi.backends import ExactIndex
    from dewi.types import Payload
    ix = ExactIndex(dim=4)
    for i in range(3):
        ix.add(f"d{i}", np.ones(4, np.float32), Payload())
    with pytest.raises(ValueError, match="do not fit int32"):
        ix.set_attributes(year=[1 << 31, 0, 0])
    with pytest.raises(ValueError, match=r"has shape \(2,\), expected \(3,\)"):
        ix.set_attributes(year=[1, 2])
    with pytest.raises(ValueError, match="at most 16 attribute columns"):
        ix.set_attributes(**{f"c{i}": [0, 0, 0] for i in range(17)})
    with pytest.raises(ValueError, match="unknown payload fields"):
        ix.attributes_from_payload("nope")
    assert ix.attribute_names() == [] and ix._corpus is None
    from dewi.where import col
    with pytest.raises(ValueError, match="unknown attribute column 'year'"):
        ix.make_filter_where(col("year") > 1)
    assert ix._corpus is None


def test_attribute_files_round_trip(tmp_path):
    from dewi.attributes import read_attribute_files, write_attribute_files
    from dewi.backends import ExactIndex
    from dewi.where import col, compile_programs
    assert read_attribute_files(tmp_path) is None
    vocab = ["a.org", "b \"quoted\".org", "ünï.org"]
    cols = [("year", "int", np.array([2020, -1, 7], np.int32), None, False),
            ("noise", "float", np.array([0.5, np.nan, -0.0], np.float32), None, True),
            ("site", "cat", np.array([2, -1, 0], np.int32), vocab, False)]
    write_attribute_files(tmp_path, cols)
    back = read_attribute_files(tmp_path)
    assert [(c[0], c[1], c[3], c[4]) for c in back] == [(c[0], c[1], c[3], c[4]) for c in cols]
    for got, want in zip(back, cols):
        assert got[2].dtype == want[2].dtype and got[2].tobytes() == want[2].tobytes()
    meta = json.loads((tmp_path / "attributes.json").read_text())
    assert meta["columns"][2]["vocabulary"] == vocab and meta["num_rows"] == 3
    # an index loaded from a folder with these files knows the schema without a device
    (tmp_path / "metadata.json").write_text(json.dumps({"dim": 4, "space": "cosine", "doc_ids": ["a", "b", "c"], "normalize": True,
                                                        "is_trained": True, "num_embeddings": 0}))
    (tmp_path / "payloads.jsonl").write_text("")
    ix = ExactIndex.load(tmp_path)
    assert ix.attribute_schema() == {"year": ("int", None), "noise": ("float", None), "site": ("cat", vocab)}
    assert compile_programs([col("site") == "ünï.org"], ix).programs[0] == [(OP["I_EQ"], 0, 2, 0)]
    (tmp_path / "attributes.json").write_text(json.dumps(dict(meta, format_version=99)))
    with pytest.raises(ValueError, match="format version 99"):
        read_attribute_files(tmp_path)


# ---------------------------------------------------------------------------------------------- the C ABI's argument errors
_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer
T, A, N = (OP["TRUE"], 0, 0, 0), (OP["AND"], 0, 0, 0), (OP["NOT"], 0, 0, 0)


def call(programs=((T,),), cols=(P, P), types=(0, 1), n=10, n_columns=None, n_programs=None, sets=P, n_set_words=4,
         masks=P, progs_null=False, lengths_null=False, lengths=None, cols_null=False, types_null=False):
    from dewi import _native as nat

    def run(lib):
        flat = [i for p in programs for i in p]
        instr = (nat.PredInstr * max(len(flat), 1))(*[nat.PredInstr(*i) for i in flat])
        lens = lengths if lengths is not None else [len(p) for p in programs]
        c_lens = (ctypes.c_int32 * max(len(lens), 1))(*lens)
        c_cols = (ctypes.c_void_p * max(len(cols), 1))(*cols)
        c_types = (ctypes.c_int32 * max(len(types), 1))(*types)
        return lib.dewi_predicate_masks(None if cols_null else c_cols, None if types_null else c_types,
                                        len(cols) if n_columns is None else n_columns, n,
                                        None if progs_null else instr, None if lengths_null else c_lens,
                                        len(programs) if n_programs is None else n_programs, sets, n_set_words, None, masks, None)
    return run


LT0, FLT1 = (OP["I_LT"], 0, 5, 0), (OP["F_LT"], 1, 5, 0)
CASES = [
    # 1. null pointers
    ("null programs", call(progs_null=True), INVALID, "null pointer"),
    ("null lengths", call(lengths_null=True), INVALID, "null pointer"),
    ("null masks", call(masks=None), INVALID, "null pointer"),
    ("null columns", call(cols_null=True), INVALID, "null pointer"),
    ("null types", call(types_null=True), INVALID, "null pointer"),
    ("null sets", call(sets=None), INVALID, "null pointer"),
    ("no columns, no sets: nothing to be null", call(cols=(), types=(), cols_null=True, types_null=True, sets=None, n_set_words=0, n=0),
     OK, None),
    # 2. counts
    ("negative rows", call(n=-1), INVALID, "bad counts: -1 rows, 2 columns, 1 programs, 4 set words"),
    ("negative columns", call(n_columns=-1), INVALID, "bad counts: 10 rows, -1 columns, 1 programs, 4 set words"),
    ("no programs", call(n_programs=0), INVALID, "bad counts: 10 rows, 2 columns, 0 programs, 4 set words"),
    ("negative set words", call(n_set_words=-2), INVALID, "bad counts: 10 rows, 2 columns, 1 programs, -2 set words"),
    # 3. unsupported sizes
    ("2^32 rows", call(n=1 << 32), UNSUPPORTED, "n_rows 4294967296 exceeds 2^32-1 rows per device"),
    ("17 columns", call(cols=(P,) * 17, types=(0,) * 17), UNSUPPORTED, "17 columns exceed DEWI_PRED_MAX_COLUMNS = 16"),
    ("257 programs", call(programs=((T,),) * 257), UNSUPPORTED, "257 programs exceed DEWI_PRED_MAX_PROGRAMS = 256"),
    # 4. columns
    ("null column", call(cols=(P, None)), INVALID, "null pointer for column 1"),
    ("column type", call(types=(0, 2)), INVALID, "unknown type 2 of column 1 (0 int32, 1 fp32)"),
    # 5. programs
    ("empty program", call(lengths=[0]), INVALID, "program 0: 0 instructions (1 .. 64)"),
    ("long program", call(programs=((T,) + (N,) * 64,)), INVALID, "program 0: 65 instructions (1 .. 64)"),
    ("unknown op", call(programs=((T,), ((22, 0, 0, 0),))), INVALID, "program 1 instruction 0: unknown op 22"),
    ("negative op", call(programs=(((-1, 0, 0, 0),),)), INVALID, "program 0 instruction 0: unknown op -1"),
    ("column out of range", call(programs=(((OP["I_EQ"], 2, 0, 0),),)), INVALID, "program 0 instruction 0: column 2 outside [0, 2)"),
    ("negative column", call(programs=((T, (OP["F_EQ"], -1, 0, 0), A),)), INVALID, "program 0 instruction 1: column -1 outside [0, 2)"),
    ("int op on a float column", call(programs=(((OP["I_LT"], 1, 0, 0),),)), INVALID,
     "program 0 instruction 0: op 0 takes an int32 column, column 1 is fp32"),
    ("float op on an int column", call(programs=(((OP["F_IS_NAN"], 0, 0, 0),),)), INVALID,
     "program 0 instruction 0: op 17 takes an fp32 column, column 0 is int32"),
    ("set outside the words", call(programs=(((OP["I_IN_SET"], 0, 3, 33),),)), INVALID,
     "program 0 instruction 0: a set of 33 bits from word 3 on lies outside the 4 set words"),
    ("set at the end of the words", call(programs=(((OP["I_IN_SET"], 0, 3, 32),),), n=0), OK, None),
    ("underflow AND", call(programs=((T, A),)), INVALID, "program 0 instruction 1: stack underflow"),
    ("underflow NOT", call(programs=((N,),)), INVALID, "program 0 instruction 0: stack underflow"),
    ("too deep", call(programs=((T,) * 33 + (A,) * 31,)), INVALID, "program 0 instruction 32: stack deeper than 32"),
    ("depth 32 is fine", call(programs=((T,) * 32 + (A,) * 31,), n=0), OK, None),
    ("two values left", call(programs=((T, T),)), INVALID, "program 0 ends with 2 values on the stack, not 1"),
    ("second program bad", call(programs=((LT0,), (LT0, FLT1))), INVALID, "program 1 ends with 2 values on the stack, not 1"),
    ("no rows", call(programs=((LT0, FLT1, A, N),), n=0), OK, None),
    # the pinned order: null pointers, counts, unsupported sizes, columns, programs (in order), then n_rows == 0
    ("order: null before counts", call(masks=None, n=-1), INVALID, "null pointer"),
    ("order: counts before unsupported", call(n=1 << 32, n_programs=0), INVALID,
     "bad counts: 4294967296 rows, 2 columns, 0 programs, 4 set words"),
    ("order: rows before columns before programs", call(n=1 << 32, cols=(P,) * 17, types=(0,) * 17, programs=((T,),) * 257), UNSUPPORTED,
     "n_rows 4294967296 exceeds 2^32-1 rows per device"),
    ("order: columns before programs", call(cols=(P,) * 17, types=(0,) * 17, programs=((T,),) * 257), UNSUPPORTED,
     "17 columns exceed DEWI_PRED_MAX_COLUMNS = 16"),
    ("order: unsupported before a null column", call(cols=(None,) + (P,) * 16, types=(0,) * 17), UNSUPPORTED,
     "17 columns exceed DEWI_PRED_MAX_COLUMNS = 16"),
    ("order: null column 0 before the type of column 0", call(cols=(None, P), types=(7, 7)), INVALID, "null pointer for column 0"),
    ("order: type of column 0 before null column 1", call(cols=(P, None), types=(7, 0)), INVALID,
     "unknown type 7 of column 0 (0 int32, 1 fp32)"),
    ("order: columns before programs' content", call(types=(0, 3), programs=((N,),)), INVALID, "unknown type 3 of column 1 (0 int32, 1 fp32)"),
    ("order: first bad program wins", call(programs=((T, T), (N,))), INVALID, "program 0 ends with 2 values on the stack, not 1"),
    ("order: length before instructions", call(programs=((N,), (T,)), lengths=[65, 1]), INVALID, "program 0: 65 instructions (1 .. 64)"),
    ("order: op before column", call(programs=(((40, 9, 0, 0),),)), INVALID, "program 0 instruction 0: unknown op 40"),
    ("order: column range before type before set", call(programs=(((OP["I_IN_SET"], 5, 9, 99),),)), INVALID,
     "program 0 instruction 0: column 5 outside [0, 2)"),
    ("order: type before set", call(programs=(((OP["I_IN_SET"], 1, 9, 99),),)), INVALID,
     "program 0 instruction 0: op 9 takes an int32 column, column 1 is fp32"),
    ("order: earlier instruction first", call(programs=((A, (40, 0, 0, 0)),)), INVALID, "program 0 instruction 0: stack underflow"),
    ("order: programs before n_rows == 0", call(programs=((T, T),), n=0), INVALID, "program 0 ends with 2 values on the stack, not 1"),
]


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,run,code,message", CASES, ids=[c[0] for c in CASES])
def test_predicate_masks_argument_error(lib, name, run, code, message):
    from dewi import _native as nat
    rc = run(lib)
    got = nat.last_error()
    print(f"{name}: rc {rc}, {got!r}")
    assert rc == code, (name, rc, got)
    if message is not None:
        assert got == message, name


def test_symbol_constants_and_struct_match_the_header(lib):
    from dewi import _native as nat
    assert "dewi_predicate_masks" in nat.EXPORTED_SYMBOLS and ctypes.sizeof(nat.PredInstr) == 16
    assert nat.PRED_OPS == pm.OPS
    header = (__import__("pathlib").Path(__file__).resolve().parent.parent / "include" / "dewi_hip.h").read_text()
    for name, code in nat.PRED_OP_CODES.items():
        assert f"#define DEWI_PRED_{name} {code}\n" in header, name
    for name, value in (("COLUMNS", nat.PRED_MAX_COLUMNS), ("INSTR", nat.PRED_MAX_INSTR), ("DEPTH", nat.PRED_MAX_DEPTH),
                        ("PROGRAMS", nat.PRED_MAX_PROGRAMS)):
        assert f"#define DEWI_PRED_MAX_{name} {value}" in header
    with pytest.raises(ValueError, match="stack underflow"):
        nat.check(call(programs=((N,),))(lib))
    with pytest.raises(NotImplementedError, match="exceed DEWI_PRED_MAX_PROGRAMS"):
        nat.check(call(programs=((T,),) * 257)(lib))

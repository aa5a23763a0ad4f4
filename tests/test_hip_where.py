"""GPU tests of metadata predicates: ``dewi_predicate_masks`` against the NumPy model (``predicate_model.py``), byte for byte,
and ``filter=<Where>`` through every layer against the same call with the model's boolean mask, bit for bit.

The C-ABI tests call the library directly.  Every column is the LAST ``n_rows`` elements of a larger buffer whose front holds
other values (a read below the start would flip results), the column pointers are only 4-byte aligned, and ``d_masks`` lies
between guard bytes (``wsguard``).  Odd ``n_rows`` with several programs are the unaligned-row cases: program p's mask starts at
byte ``p * n_rows``.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import predicate_model as pm
import wsguard as wsg
from predicate_model import OP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 37                                   # elements in front of every column: its pointer is 4-byte aligned, no more


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library()


def run_masks(lib, cols, pad, programs, sets, base, n, prefill="0xff", check=True):
    """``dewi_predicate_masks`` on columns given as host arrays of ``pad + n`` elements -> host bytes [P, n]."""
    from dewi import _native as nat
    torch.cuda.set_device(0)
    dev_cols = [torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in cols]
    ptrs = (ctypes.c_void_p * max(len(cols), 1))(*[t.data_ptr() + 4 * pad for t in dev_cols])
    types = (ctypes.c_int32 * max(len(cols), 1))(*[1 if c.dtype == np.float32 else 0 for c in cols])
    flat = [i for p in programs for i in p]
    instr = (nat.PredInstr * len(flat))(*[nat.PredInstr(*i) for i in flat])
    lens = (ctypes.c_int32 * len(programs))(*[len(p) for p in programs])
    d_sets = torch.from_numpy(np.ascontiguousarray(sets, dtype=np.uint32).view(np.int32)).to(DEV)
    d_base = None if base is None else torch.from_numpy(np.ascontiguousarray(base, dtype=np.uint8)).to(DEV)
    out = wsg.GuardedBuffer(len(programs) * n, DEV, prefill, label="d_masks")
    nat.check(lib.dewi_predicate_masks(ptrs, types, len(cols), n, instr, lens, len(programs),
                                       d_sets.data_ptr() if d_sets.numel() else None, d_sets.numel(),
                                       None if d_base is None else d_base.data_ptr(), out.view.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if check:
        out.check(interior=False)          # the guards in front of and behind d_masks are untouched
    return out.view.cpu().numpy().reshape(len(programs), n)


def model_masks(cols, pad, programs, sets, base):
    types = [1 if c.dtype == np.float32 else 0 for c in cols]
    tail = [c[pad:] for c in cols]
    return np.stack([pm.evaluate(tail, types, p, sets, base) for p in programs])


def edge_columns(rs, n, pad, types=(0, 1, 0, 1)):
    cols = [pm.edge_column(rs, n, t, pad) for t in types]
    for c, t in zip(cols, types):          # the edge values are there at every size, the last row included
        edges = pm.FLOAT_EDGES if t else pm.INT_EDGES
        m = min(n, len(edges))
        c[pad + n - m:] = edges[:m]
    return cols


# ------------------------------------------------------------------------------------------------------- 1. the ABI sweep
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 1000, 4099, 65537])
def test_abi_sweep_equals_the_model(lib, n):
    rs = np.random.RandomState(n)
    cols = edge_columns(rs, n, PAD)
    sets, table = pm.random_sets(rs)
    base = (rs.rand(n) < 0.6).astype(np.uint8) * rs.randint(1, 256, n).astype(np.uint8)      # non-zero = allowed, any byte
    types = [1 if c.dtype == np.float32 else 0 for c in cols]
    depths, lengths = [], []
    for n_programs in (1, 2, 5, 33):
        programs = [pm.random_program(rs, types, table, length=(1 if n_programs == 1 and n % 2 else None)) for _ in range(n_programs)]
        if n_programs == 33:
            programs[0] = pm.random_program(rs, types, table, length=64)
            programs[-1] = pm.random_program(rs, types, table, length=1)
        lengths += [len(p) for p in programs]
        want = model_masks(cols, PAD, programs, sets, None)
        got = run_masks(lib, cols, PAD, programs, sets, None, n)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (n, n_programs, "no base")
        # the same rows behind a front of 32 elements: 16-byte aligned columns (the run above: 4-byte aligned, no more)
        aligned = [np.ascontiguousarray(c[PAD - 32:]) for c in cols]
        got = run_masks(lib, aligned, 32, programs, sets, base, n, prefill="zeros")
        assert np.array_equal(got, want & (base != 0)), (n, n_programs, "base")
    assert min(lengths) == 1 and max(lengths) == 64


def test_abi_sweep_reaches_depth_32_and_every_op(lib):
    from dewi.where import program_depth
    rs = np.random.RandomState(7)
    n = 257
    cols = edge_columns(rs, n, PAD)
    sets, table = pm.random_sets(rs)
    types = [1 if c.dtype == np.float32 else 0 for c in cols]
    programs = [pm.random_program(rs, types, table, length=64) for _ in range(120)]
    assert max(program_depth(p) for p in programs) == 32
    assert {i[0] for p in programs for i in p} == set(range(len(pm.OPS)))
    assert np.array_equal(run_masks(lib, cols, PAD, programs, sets, None, n), model_masks(cols, PAD, programs, sets, None))


# ------------------------------------------------------------------------------------------------------- 2. I_IN_SET
def test_in_set_bounds_offsets_and_poison(lib):
    n = 300
    x = np.zeros(PAD + n, dtype=np.int32)
    x[:PAD] = 3                                                                 # in front of the column: members of every set
    tail = np.arange(-20, n - 20, dtype=np.int32)
    tail[:6] = [-1, -(1 << 31), (1 << 31) - 1, 1 << 24, 100, 127]
    x[PAD:] = tail
    rs = np.random.RandomState(3)
    sets, table = pm.random_sets(rs, n_sets=5)
    assert any(b % 32 for _, b in table) and len({a for a, _ in table}) == 5
    # a set of 33 bits whose second word has bits set BEYOND bit 32: x == 33 .. 63 must not be members
    words = np.concatenate([sets, np.array([0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)])
    table = table + [(len(sets), 33), (len(sets) + 1, 1), (len(words) - 1, 32), (0, 0)]
    programs = [[(OP["I_IN_SET"], 0, a, b)] for a, b in table]
    programs.append([(OP["I_IN_SET"], 0, a, b) for a, b in table[:4]] + [(OP["OR"], 0, 0, 0)] * 3 + [(OP["NOT"], 0, 0, 0)])
    want = model_masks([x], PAD, programs, words, None)
    got = run_masks(lib, [x], PAD, programs, words, None, n)
    assert np.array_equal(got, want)
    k = len(sets)
    at = {int(v): i for i, v in enumerate(tail)}
    p33 = got[5]                                                                # the 33-bit set of all-ones words
    assert p33[at[0]] == 1 and p33[at[32]] == 1 and p33[at[33]] == 0 and p33[at[63]] == 0 and p33[at[-1]] == 0
    assert p33[2] == 0 and p33[1] == 0                                          # INT32_MAX, INT32_MIN
    assert got[8].sum() == 0                                                    # a set of 0 bits
    assert k > 0


# ------------------------------------------------------------------------------------------------------- 3. launch split
@pytest.mark.parametrize("n_programs", [33, 256])
def test_many_long_programs_equal_one_per_call(lib, n_programs):
    rs = np.random.RandomState(n_programs)
    n = 1001
    cols = edge_columns(rs, n, PAD)
    sets, table = pm.random_sets(rs)
    types = [1 if c.dtype == np.float32 else 0 for c in cols]
    programs = [pm.random_program(rs, types, table, length=64) for _ in range(n_programs)]
    base = (rs.rand(n) < 0.8).astype(np.uint8)
    got = run_masks(lib, cols, PAD, programs, sets, base, n)                    # several launches: 4 programs of 64 fit one
    for p in range(n_programs):
        one = run_masks(lib, cols, PAD, programs[p: p + 1], sets, base, n, check=False)
        assert np.array_equal(got[p], one[0]), p
    assert np.array_equal(got, model_masks(cols, PAD, programs, sets, base))


def test_more_rows_than_one_trip_of_the_grid(lib):
    n = 1_048_583
    rs = np.random.RandomState(11)
    cols = edge_columns(rs, n, PAD, types=(0, 1, 0))
    sets, table = pm.random_sets(rs)
    programs = [[(OP["I_GE"], 0, 20, 0), (OP["F_LT"], 1, 0x3F000000, 0), (OP["AND"], 0, 0, 0), (OP["I_IN_SET"], 2, *table[0]),
                 (OP["OR"], 0, 0, 0)],
                [(OP["F_IS_NAN"], 1, 0, 0), (OP["NOT"], 0, 0, 0)],
                [(OP["I_ANY_BITS"], 2, 5, 0)]]
    want = model_masks(cols, PAD, programs, sets, None)
    got = run_masks(lib, cols, PAD, programs, sets, None, n)
    assert np.array_equal(got, want)
    assert 0 < want[0, n - 600:].sum() < 600                                    # the rows of the last trip are not trivial


# ------------------------------------------------------------------------------------------------------- 4. determinism
def test_same_bytes_twice_and_whatever_the_output_held(lib):
    rs = np.random.RandomState(13)
    n = 4099
    cols = edge_columns(rs, n, PAD)
    sets, table = pm.random_sets(rs)
    types = [1 if c.dtype == np.float32 else 0 for c in cols]
    programs = [pm.random_program(rs, types, table) for _ in range(7)]
    base = (rs.rand(n) < 0.5).astype(np.uint8)
    runs = [run_masks(lib, cols, PAD, programs, sets, base, n, prefill=f) for f in ("zeros", "0xff", "0xff", "random")]
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])                                       # every byte is written: the prefill never shows
    assert set(np.unique(runs[0])) <= {0, 1}


# ------------------------------------------------------------------------------------------------------- 5. through the layers
N, D, K = 8192, 64, 7
ETA, PREF = 0.4, 0.1
_world = {}


def world():
    """The corpus, its attributes on the host, and the three indexes — built once."""
    if _world:
        return _world
    import dewi_oracle as orc
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    from dewi.types import payloads_from_columns
    rs = np.random.RandomState(21)
    raw = orc.synth_corpus(N, D, seed=5)
    pay = orc.synth_payload_columns(N, seed=5)
    ids = [f"doc_{i:05d}" for i in range(N)]
    sites = [f"site{j}.org" for j in range(40)]
    site = [None if rs.rand() < 0.05 else sites[int(rs.randint(40))] for _ in range(N)]
    score = rs.randn(N).astype(np.float64)
    score[rs.rand(N) < 0.1] = np.nan
    attrs = {"year": rs.randint(1990, 2026, N).astype(np.int64), "tags": rs.randint(0, 16, N).astype(np.int32),
             "site": site, "score": score}
    payloads = payloads_from_columns(pay)
    exact = ExactIndex(dim=D, int8_shadow=True)
    exact.add_batch(ids, raw, payloads)
    ivf = IVFIndex(dim=D, nlist=16, train_iters=3, int8_codes=True)
    ivf.add_batch(ids, raw, payloads)
    facade = DewiIndex(dim=D, use_ann=False, rerank_eta=ETA, entropy_pref=PREF)
    facade.add_batch(ids, raw, payloads)
    for ix in (exact, ivf, facade):
        ix.build()
        ix.set_attributes(**attrs)
        ix.attributes_from_payload("noise", "dewi")
    vocab = sorted(set(s for s in site if s is not None))
    code = {s: i for i, s in enumerate(vocab)}
    host = {"year": attrs["year"].astype(np.int32), "tags": attrs["tags"], "score": score.astype(np.float32),
            "site": np.array([-1 if s is None else code[s] for s in site], dtype=np.int32),
            "noise": pay["noise"].astype(np.float32), "dewi": pay["dewi"].astype(np.float32)}
    _world.update(raw=raw, pay=pay, ids=ids, attrs=attrs, host=host, vocab=vocab, exact=exact, ivf=ivf, facade=facade,
                  Q=orc.synth_queries(16, D, seed=3))
    return _world


def model_mask(w, where):
    """The model's boolean mask of a ``Where``: compiled against the index's schema, evaluated on the host columns."""
    from dewi.where import compile_programs
    p = compile_programs([where], w["exact"])
    cols = [w["host"][name] for name in p.columns]
    return pm.evaluate(cols, [1 if c.dtype == np.float32 else 0 for c in cols], p.programs[0], p.sets).astype(bool)


def wheres():
    from dewi.where import col
    return {
        "issue": (col("year") >= 2020) & col("site").isin([f"site{j}.org" for j in range(0, 40, 3)]) & (col("noise") < 0.2),
        "or-not": (col("tags").any_bits(0b1010) | ~(col("score") < 0.0)) & (col("dewi").between(0.2, 0.9)),
        "nan": col("score").isnan() | (col("site") == None),                    # noqa: E711
        "narrow": (col("year") == 2001) & col("tags").all_bits(3),
    }


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) and np.shape(x) == np.shape(y)
               for x, y in zip(a, b)) and len(a) == len(b)


def test_attributes_are_what_was_set():
    w = world()
    for ix in (w["exact"], w["ivf"], w["facade"]):
        assert ix.attribute_names() == ["year", "tags", "site", "score", "noise", "dewi"]
        got = ix.attributes_of(w["ids"][:50] + w["ids"][-3:])
        rows = list(range(50)) + [N - 3, N - 2, N - 1]
        for name in ("year", "tags", "noise", "dewi", "score"):
            assert got[name].tobytes() == w["host"][name][rows].tobytes(), name
        assert got["site"] == [w["attrs"]["site"][r] for r in rows]
    schema = w["exact"].attribute_schema()
    assert schema["site"] == ("cat", w["vocab"]) and schema["year"][0] == "int" and schema["noise"][0] == "float"


@pytest.mark.parametrize("name", ["issue", "or-not", "nan", "narrow"])
def test_search_with_a_where_equals_the_models_mask(name):
    w = world()
    where = wheres()[name]
    mask = model_mask(w, where)
    assert 0 < mask.sum() < N
    Q = w["Q"]
    for ix in (w["exact"], w["ivf"]):
        assert ix.count_where(where) == int(mask.sum())
        f = ix.make_filter_where(where)
        assert len(f) == int(mask.sum()) and np.array_equal(f.byte_mask().cpu().numpy().astype(bool), mask)
        assert same(ix.search_batch(Q, K, ETA, PREF, filter=where), ix.search_batch(Q, K, ETA, PREF, filter=mask))
        assert same(ix.search_batch(Q[:1], K, ETA, PREF, filter=f), ix.search_batch(Q[:1], K, ETA, PREF, filter=mask))
        a, b = ix.search(Q[0], K, ETA, PREF, filter=where), ix.search(Q[0], K, ETA, PREF, filter=mask)
        assert [(r[0], np.float32(r[1]).tobytes()) for r in a] == [(r[0], np.float32(r[1]).tobytes()) for r in b] and len(a) == K
        assert same(ix.range_search_batch(Q[:4], 0.1, ETA, PREF, filter=where), ix.range_search_batch(Q[:4], 0.1, ETA, PREF, filter=mask))
    fa = w["facade"]
    assert fa.count_where(where) == int(mask.sum())
    a, b = fa.search_batch(Q, K, filter=where), fa.search_batch(Q, K, filter=mask)
    assert [[(r[0], np.float32(r[1]).tobytes()) for r in row] for row in a] == [[(r[0], np.float32(r[1]).tobytes()) for r in row] for row in b]
    a, b = fa.search(Q[1], K, filter=where), fa.search(Q[1], K, filter=mask)
    assert [(r[0], r[1]) for r in a] == [(r[0], r[1]) for r in b]
    assert [r[0] for r in fa.range_search(Q[0], 0.1, filter=where)] == [r[0] for r in fa.range_search(Q[0], 0.1, filter=mask)]


def test_other_routes_take_a_where():
    w = world()
    where = wheres()["issue"]
    mask = model_mask(w, where)
    Q, exact, ivf = w["Q"], w["exact"], w["ivf"]
    groups = w["host"]["site"]
    for ix in (exact, ivf):
        assert same(ix.search_collapsed_batch(Q[:4], K, ETA, PREF, groups=groups, filter=where),
                    ix.search_collapsed_batch(Q[:4], K, ETA, PREF, groups=groups, filter=mask))
        assert ix.select_subset(20, filter=where) == ix.select_subset(20, filter=mask)
        assert ix.select_subset_blocked(20, filter=where) == ix.select_subset_blocked(20, filter=mask)
    assert same(exact.search_approx_filtered_batch(Q, K, ETA, PREF, filter=where),
                exact.search_approx_filtered_batch(Q, K, ETA, PREF, filter=mask))
    for approx in (False, True):
        assert same(ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=where, nprobe=4, approx=approx),
                    ivf.search_probe_filtered_batch(Q, K, ETA, PREF, filter=mask, nprobe=4, approx=approx))
    # a base filter is ANDed in: dedup_filter composes with a predicate
    dedup = exact.dedup_filter(0.45)
    dmask = dedup.byte_mask().cpu().numpy().astype(bool)
    assert 0 < (dmask & mask).sum() < mask.sum()
    f = exact.make_filter_where(where, base=dedup)
    assert np.array_equal(f.byte_mask().cpu().numpy().astype(bool), dmask & mask) and len(f) == int((dmask & mask).sum())
    assert same(exact.search_batch(Q, K, ETA, PREF, filter=f), exact.search_batch(Q, K, ETA, PREF, filter=dmask & mask))
    with pytest.raises(TypeError):
        exact.make_filter_where(where, base=mask)
    with pytest.raises(ValueError, match="another corpus"):
        exact.make_filter_where(where, base=ivf.make_filter(mask))


def test_per_query_wheres_equal_make_query_filters_of_the_models_masks():
    from dewi.where import col
    w = world()
    Q, exact, ivf = w["Q"], w["exact"], w["ivf"]
    ws = [wheres()[name] for name in ("issue", "or-not", "nan", "narrow")] * 2 + [col("year") > 3000]     # the last one: nothing
    masks = np.stack([model_mask(w, x) for x in ws])
    b = len(ws)
    for ix in (exact, ivf):
        qf = ix.make_query_filters_where(ws)
        assert qf.n_queries == b and qf.n_allowed.tolist() == masks.sum(axis=1).tolist() and qf.n_union == int(masks.any(axis=0).sum())
        want = ix.search_batch(Q[:b], K, ETA, PREF, filter=ix.make_query_filters(masks))
        assert same(ix.search_batch(Q[:b], K, ETA, PREF, filter=ws), want)
        assert same(ix.search_batch(Q[:b], K, ETA, PREF, filter=qf), want)
        assert (want[0][-1] == -1).all()                                                                    # the empty list pads its row
    assert same(ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=ws, nprobe=4),
                ivf.search_probe_filtered_batch(Q[:b], K, ETA, PREF, filter=masks, nprobe=4))
    assert same(exact.search_approx_filtered_batch(Q[:b], K, ETA, PREF, filter=ws),
                exact.search_approx_filtered_batch(Q[:b], K, ETA, PREF, filter=masks))
    res = w["facade"].search_batch(Q[:b], K, filter=ws)
    assert res[-1] == [] and all(len(r) == K for r in res[:-1])
    with pytest.raises(NotImplementedError):
        exact.range_search_batch(Q[:b], 0.1, filter=ws)
    with pytest.raises(NotImplementedError):
        exact.search_collapsed_batch(Q[:b], K, groups=w["host"]["site"], filter=ws)
    with pytest.raises(ValueError, match="one allow-list"):
        exact.select_subset(5, filter=ws)


def test_nothing_matches_and_k_above_the_list():
    from dewi.where import col
    w = world()
    Q = w["Q"]
    nothing = (col("year") > 3000) | (col("site") == "nowhere.org")
    few = (col("year") == 2001) & col("tags").all_bits(7)
    n_few = int(model_mask(w, few).sum())
    assert 0 < n_few < 200
    for ix in (w["exact"], w["ivf"], w["facade"]):
        assert ix.count_where(nothing) == 0 and ix.search(Q[0], K, filter=nothing) == []
        assert len(ix.make_filter_where(nothing)) == 0
        with pytest.raises(ValueError) as by_where:
            ix.search(Q[0], n_few + 1, filter=few)
        with pytest.raises(ValueError) as by_mask:
            ix.search(Q[0], n_few + 1, filter=model_mask(w, few))
        assert str(by_where.value) == str(by_mask.value)
        assert len(ix.search(Q[0], n_few, filter=few)) == n_few
    rows, scores = w["exact"].search_batch(Q[:3], K, filter=nothing)
    assert rows.shape == (3, 0) and scores.shape == (3, 0)


def test_errors_of_the_attribute_methods():
    from dewi.where import col
    w = world()
    ix = w["exact"]
    with pytest.raises(ValueError, match="unknown attribute columns"):
        ix.update_attributes(w["ids"][:2], nope=[1, 2])
    with pytest.raises(ValueError, match="unknown attribute columns"):
        ix.drop_attributes("nope")
    with pytest.raises(KeyError):
        ix.update_attributes(["no such doc"], year=1)
    with pytest.raises(ValueError, match="do not fit int32"):
        ix.update_attributes(w["ids"][:1], year=[1 << 40])
    with pytest.raises(ValueError, match="holds integers, got floats"):
        ix.update_attributes(w["ids"][:1], year=[0.5])
    with pytest.raises(ValueError, match="values for 2 documents"):
        ix.update_attributes(w["ids"][:2], year=[1, 2, 3])
    with pytest.raises(ValueError, match="unknown attribute column 'nope'"):
        ix.search(w["Q"][0], K, filter=col("nope") > 1)
    with pytest.raises(ValueError, match="not categorical"):
        ix.count_where(col("year") == "site3.org")
    assert ix.attributes_of(w["ids"][:1])["year"].tolist() == [int(w["host"]["year"][0])]                     # nothing was written


# ------------------------------------------------------------------------------------------------------- 6. mutation and files
def _mutated():
    """An index that went through remove / upsert (known and new ids) / update_attributes / reserve, and the host's model of
    it: ``{doc_id: (raw row, payload columns, attributes)}``."""
    import dewi_oracle as orc
    from dewi.backends import ExactIndex
    from dewi.types import payloads_from_columns
    from dewi.where import col
    n0, d = 2000, 64
    rs = np.random.RandomState(31)
    raw = orc.synth_corpus(n0 + 60, d, seed=9)
    pay = orc.synth_payload_columns(n0 + 60, seed=9)
    plist = payloads_from_columns(pay)
    ids = [f"d{i:04d}" for i in range(n0 + 60)]
    year = rs.randint(1990, 2026, n0 + 60)
    site = [None if rs.rand() < 0.1 else f"s{int(rs.randint(9))}" for _ in range(n0 + 60)]
    temp = rs.randn(n0 + 60).astype(np.float32)
    model = {ids[i]: {"row": i, "year": int(year[i]), "site": site[i], "temp": np.float32(temp[i])} for i in range(n0)}
    ix = ExactIndex(dim=d)
    ix.add_batch(ids[:n0], raw[:n0], plist[:n0])
    ix.build()
    ix.set_attributes(year=year[:n0], site=site[:n0], temp=temp[:n0])
    ix.attributes_from_payload("noise")
    before = ix.make_filter_where(col("year") > 2000)
    # remove
    gone = [ids[i] for i in rs.choice(n0, 100, replace=False)]
    ix.remove(gone)
    for g in gone:
        del model[g]
    # upsert: 40 known ids take the embedding and payload of other source rows and KEEP their attributes; 60 new ids are
    # appended with the fills
    known = [d_ for d_ in ids[:n0] if d_ in model][5:45]
    src = list(range(n0 - 40, n0))
    new = list(range(n0, n0 + 60))
    ix.reserve(2100)
    ix.upsert_batch(known + [ids[i] for i in new], raw[src + new], [plist[i] for i in src + new])
    for d_, s in zip(known, src):
        model[d_]["row"] = s
    for i in new:
        model[ids[i]] = {"row": i, "year": 0, "site": None, "temp": np.float32(np.nan)}
    filled = ix.attributes_of([ids[i] for i in new[:3]])
    assert filled["year"].tolist() == [0, 0, 0] and filled["site"] == [None] * 3 and np.isnan(filled["temp"]).all()
    # the user gives the new documents their attributes; "zz" is a word the vocabulary did not have
    upd = [ids[i] for i in new[:50]]
    ix.update_attributes(upd, year=[int(year[i]) for i in new[:50]], site=["zz" if i % 7 == 0 else site[i] for i in new[:50]],
                         temp=temp[new[:50]])
    for i in new[:50]:
        model[ids[i]].update(year=int(year[i]), site="zz" if i % 7 == 0 else site[i], temp=np.float32(temp[i]))
    ix.update_attributes(known[:4], year=1234)                                  # one value for all of them
    for d_ in known[:4]:
        model[d_]["year"] = 1234
    ix.reserve(5000)
    return ix, model, raw, pay, plist, before


def test_attributes_follow_remove_upsert_update_reserve(tmp_path):
    from dewi.backends import ExactIndex
    from dewi.where import col
    ix, model, raw, pay, plist, before = _mutated()
    order = list(ix._doc_ids)
    assert sorted(order) == sorted(model) and ix.capacity >= 5000
    got = ix.attributes_of(order)
    assert got["year"].tolist() == [model[d]["year"] for d in order]
    assert got["site"] == [model[d]["site"] for d in order]
    assert got["temp"].tobytes() == np.array([model[d]["temp"] for d in order], np.float32).tobytes()
    assert got["noise"].tobytes() == np.array([pay["noise"][model[d]["row"]] for d in order], np.float32).tobytes()   # the mirror followed
    assert "zz" in ix.attribute_schema()["site"][1] and ix.attribute_schema()["site"][1] == sorted(ix.attribute_schema()["site"][1])
    # a filter prepared before the mutations is refused
    with pytest.raises(ValueError, match="another corpus"):
        ix.search(raw[0], 3, filter=before)
    # a freshly built index with the same documents and attributes answers the same, bit for bit
    rows = [model[d]["row"] for d in order]
    fresh = ExactIndex(dim=64)
    fresh.add_batch(order, raw[rows], [plist[r] for r in rows])
    fresh.build()
    fresh.set_attributes(year=[model[d]["year"] for d in order], site=[model[d]["site"] for d in order],
                         temp=np.array([model[d]["temp"] for d in order], np.float32))
    fresh.attributes_from_payload("noise")
    Q = raw[[3, 500, 1999, 2040]] + 0.05
    for where in ((col("year") >= 2005) & (col("noise") < 0.15), col("site").isin(["zz", "s3", None]) | col("temp").isnan(),
                  ~(col("temp") > 0.0) & (col("year") != 1234)):
        assert 0 < ix.count_where(where) == fresh.count_where(where) < len(order)
        assert same(ix.search_batch(Q, 6, ETA, PREF, filter=where), fresh.search_batch(Q, 6, ETA, PREF, filter=where))
    # files: attributes round-trip, metadata.json is what a save without attributes writes
    ix.save(tmp_path / "with")
    plain = ExactIndex(dim=64)
    plain.add_batch(order, raw[rows], [plist[r] for r in rows])
    plain.build()
    plain.save(tmp_path / "without")
    assert (tmp_path / "with" / "metadata.json").read_bytes() == (tmp_path / "without" / "metadata.json").read_bytes()
    assert not (tmp_path / "without" / "attributes.json").exists() and not (tmp_path / "without" / "attributes.npz").exists()
    names = json.loads((tmp_path / "with" / "attributes.json").read_text())
    assert [c["name"] for c in names["columns"]] == ["year", "site", "temp", "noise"]
    back = ExactIndex.load(tmp_path / "with")
    assert back.attribute_schema() == ix.attribute_schema()                     # known before anything is on the device
    again = back.attributes_of(order)
    for name in ("year", "temp", "noise"):
        assert again[name].tobytes() == got[name].tobytes()
    assert again["site"] == got["site"]
    where = (col("year") >= 2005) & (col("site") != "zz")
    assert same(back.search_batch(Q, 6, ETA, PREF, filter=where), ix.search_batch(Q, 6, ETA, PREF, filter=where))
    assert ExactIndex.load(tmp_path / "without").attribute_names() == []
    # a loaded index whose first act is a mutation: the attributes go to the device before the rows move
    back2 = ExactIndex.load(tmp_path / "with")
    back2.remove(order[:5])
    assert back2.attributes_of(order[5:9])["year"].tolist() == [model[d]["year"] for d in order[5:9]]


def test_ivf_index_keeps_attributes_through_mutation_and_files(tmp_path):
    import dewi_oracle as orc
    from dewi.ivf import IVFIndex
    from dewi.types import payloads_from_columns
    from dewi.where import col
    n, d = 3000, 64
    raw = orc.synth_corpus(n + 10, d, seed=17)
    plist = payloads_from_columns(orc.synth_payload_columns(n + 10, seed=17))
    ids = [f"d{i:04d}" for i in range(n + 10)]
    year = np.random.RandomState(1).randint(1990, 2026, n + 10)
    ivf = IVFIndex(dim=d, nlist=8, train_iters=3)
    ivf.add_batch(ids[:n], raw[:n], plist[:n])
    ivf.build()
    ivf.set_attributes(year=year[:n])
    ivf.remove(ids[10:200])
    ivf.upsert_batch(ids[n:], raw[n:], plist[n:])
    ivf.update_attributes(ids[n:], year=year[n:])
    order = list(ivf._doc_ids)
    want = [int(year[int(x[1:])]) for x in order]
    assert ivf.attributes_of(order)["year"].tolist() == want
    where = col("year").between(2000, 2010)
    mask = np.array([2000 <= y <= 2010 for y in want])
    Q = raw[:5] + 0.05
    assert same(ivf.search_probe_filtered_batch(Q, 5, ETA, PREF, filter=where, nprobe=3),
                ivf.search_probe_filtered_batch(Q, 5, ETA, PREF, filter=mask, nprobe=3))
    ivf.save(tmp_path / "ivf")
    back = IVFIndex.load(tmp_path / "ivf")
    assert back.attributes_of(order)["year"].tolist() == want
    assert same(back.search_batch(Q, 5, ETA, PREF, filter=where), ivf.search_batch(Q, 5, ETA, PREF, filter=mask))

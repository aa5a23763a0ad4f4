"""GPU tests of in-place removal and upsert: the two kernels at the ABI, bit for bit against tests/mutate_model.py and against
the ingest kernels; then ``ExactIndex`` / ``DewiIndex`` / ``IVFIndex`` against an index built AFRESH from the same documents
in the mutated index's row order — stored matrix, bf16 shadow, payload columns and every search, bit for bit.

Shapes.  Kernels: n = 300 rows (75 workgroups of four wavefronts when every row moves; 299 of 300 removed is one), dims 3
(rows of 12 bytes), 50 (200 bytes: dword path), 132 and 136 (whole 16-byte units, one and more than one per lane ... 33 and 34
units: a ragged last pass of the lane loop), 768 (three units per lane); bases: an aligned allocation, row 3 of a larger
buffer (unaligned rows for dims 3 and 50) and one element into a buffer (every 16-byte unit straddles: the element paths for
dims 132, 136, 768 too).  Index: 1 000 documents; the shadow route needs 65 536 x 136, its smallest shape.
"""
import ctypes
import functools

import numpy as np
import pytest

import ivf_model
import mutate_model as mm

pytestmark = pytest.mark.gpu

N = 300
DIMS = [3, 50, 132, 136, 768]
BASES = ["aligned", "row3", "elem1"]


def _i32(t):
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy()


def _i16(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy()


def _carve(n_rows, dim, dtype, base):
    """A contiguous [n_rows, dim] view of a larger zeroed buffer: at its start, at its row 3, or one element in -> (buffer, view)."""
    import torch
    big = torch.zeros((n_rows + 5) * dim + 8, dtype=dtype, device="cuda")
    off = {"aligned": 0, "row3": 3 * dim, "elem1": 1}[base]
    return big, big[off:off + n_rows * dim].view(n_rows, dim)


# ---------------------------------------------------------------------------------------------------- dewi_rows_move
def _removal_sets():
    rs = np.random.RandomState(3)
    sets = {"one middle row": [150], "the first row": [0], "the last row": [N - 1], "the first 100": list(range(100)),
            "the last 100": list(range(N - 100, N)), "every other row": list(range(0, N, 2)),
            "299 of 300": [r for r in range(N) if r != 17]}
    for s in range(5):
        sets[f"random {s}"] = rs.choice(N, int(rs.randint(2, N - 1)), replace=False).tolist()
    return sets


class _MoveArrays:
    """Matrix (every element its own int32 pattern, every fifth row NaN patterns), shadow (16-bit patterns), payload and aux
    columns, each inside a larger buffer whose every byte is compared afterwards."""

    def __init__(self, dim, base, elem=0):
        import torch
        self.dim, self.elem = dim, elem
        pat = np.arange(N * dim, dtype=np.int64).reshape(N, dim)
        pat[::5] |= 0x7FC00000                                             # quiet NaNs with a payload: moved as bits
        sh = ((np.arange(N)[:, None] * 131 + np.arange(dim)[None, :] * 7 + 1) & 0xFFFF).astype(np.uint16).view(np.int16)
        if elem == 0:
            self.big_e, self.E = _carve(N, dim, torch.int32, base)
            self.E.copy_(torch.from_numpy(pat.astype(np.int32)))
            self.big_s, self.S = _carve(N, dim, torch.int16, base)
            self.S.copy_(torch.from_numpy(sh))
        else:                                                              # a bf16 main matrix: 2-byte elements, no shadow
            self.big_e, self.E = _carve(N, dim, torch.int16, base)
            self.E.copy_(torch.from_numpy(sh))
            self.big_s = self.S = None
        self.cols = torch.zeros((3, N + 4), dtype=torch.int32, device="cuda")
        self.cols[0, :N] = torch.arange(N, dtype=torch.int32) + 100000      # dewi32, ent32 (as bit patterns), aux
        self.cols[1, :N] = torch.arange(N, dtype=torch.int32) + 200000
        self.cols[2, :N] = torch.arange(N, dtype=torch.int32) + 300000
        self.err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def snapshot(self):
        return [t.clone() for t in (self.big_e, self.big_s, self.cols) if t is not None]

    def move(self, src, dst, n_keep, aux=True):
        import torch
        from dewi import _native as nat
        lib = nat.load_library()
        s = torch.from_numpy(np.asarray(src, dtype=np.int64)).cuda()
        d = torch.from_numpy(np.asarray(dst, dtype=np.int64)).cuda()
        nat.check(lib.dewi_rows_move(self.E.data_ptr(), self.elem, 0 if self.S is None else self.S.data_ptr(),
                                     self.cols[0].data_ptr(), self.cols[1].data_ptr(), self.cols[2].data_ptr() if aux else 0,
                                     N, self.dim, n_keep, nat.ptr(s), nat.ptr(d), len(src), nat.ptr(self.err), nat.stream_ptr()))
        return int(self.err.item())

    def expected(self, before, src, dst, aux=True):
        """The model applied to the snapshot: destination rows take the source bits in every array; nothing else changes."""
        import torch
        want = [t.clone() for t in before]
        si = torch.tensor(src, dtype=torch.int64, device="cuda")
        di = torch.tensor(dst, dtype=torch.int64, device="cuda")
        views = [(want[0], self.big_e, self.E)] + ([(want[1], self.big_s, self.S)] if self.S is not None else [])
        for w, big, view in views:
            off = (view.data_ptr() - big.data_ptr()) // big.element_size()
            wv = w[off:off + N * self.dim].view(N, self.dim)
            wv[di] = wv[si]
        cols = want[-1]
        for c in range(3 if aux else 2):
            cols[c, di] = cols[c, si]
        return want


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("dim", DIMS)
def test_rows_move_moves_the_bits_of_every_array_and_nothing_else(dim, base):
    import torch
    for name, dele in _removal_sets().items():
        a = _MoveArrays(dim, base)
        before = a.snapshot()
        movers, holes, n_keep = mm.remove_pairs(N, dele)
        bad = a.move(movers, holes, n_keep)
        assert bad == 0, (name, bad)
        for got, want, what in zip(a.snapshot(), a.expected(before, movers, holes), ("matrix", "shadow", "columns")):
            assert torch.equal(got, want), f"dim {dim}, {base}, {name}: {what} differs"
        # the survivors in model order: the first n_keep rows ARE the old rows mm.remove_order names
        order = torch.from_numpy(mm.remove_order(N, dele)).cuda()
        off = (a.E.data_ptr() - a.big_e.data_ptr()) // 4
        old = before[0][off:off + N * dim].view(N, dim)
        assert torch.equal(a.E[:n_keep], old[order]), (name, "row order")


@pytest.mark.parametrize("dim", [50, 136])
def test_rows_move_of_a_bf16_main_matrix_and_without_aux(dim):
    import torch
    dele = _removal_sets()["random 1"]
    movers, holes, n_keep = mm.remove_pairs(N, dele)
    a = _MoveArrays(dim, "row3", elem=1)
    before = a.snapshot()
    assert a.move(movers, holes, n_keep, aux=False) == 0
    for got, want in zip(a.snapshot(), a.expected(before, movers, holes, aux=False)):
        assert torch.equal(got, want)


def test_rows_move_skips_and_counts_pairs_outside_the_contract():
    import torch
    n_keep = 290                                                 # ten rows above it: six pairs are within the call's limits
    a = _MoveArrays(132, "aligned")
    before = a.snapshot()
    src = [296, 289, 297, N, 299, 295]                           # 289 < n_keep, N outside the rows
    dst = [1, 4, n_keep, 200, 200, -1]                           # n_keep and -1 are no destinations
    assert a.move(src, dst, n_keep) == 4
    for got, want in zip(a.snapshot(), a.expected(before, [296, 299], [1, 200])):
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------- dewi_rows_put_f32
M_PUT, CAP = 40, 64


@functools.lru_cache(maxsize=None)
def _put_reference(dim, normalize):
    """What a fresh build stores for the raw rows: the ingest kernels on a fresh (aligned) allocation."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    rs = np.random.RandomState(dim)
    raw = rs.standard_normal((M_PUT, dim)).astype(np.float32)
    raw[11] = 0.0                                                # a zero row: NaN once normalised
    trip = rs.standard_normal((3, M_PUT))
    x = torch.from_numpy(raw).cuda()
    e = x.clone()
    if normalize:
        nat.check(lib.dewi_normalize_rows_f32(nat.ptr(e), nat.ptr(e), M_PUT, dim, nat.stream_ptr()))
    h = torch.empty((M_PUT, dim), dtype=torch.bfloat16, device="cuda")
    nat.check(lib.dewi_convert_f32_to_bf16(nat.ptr(e), nat.ptr(h), e.numel(), nat.stream_ptr()))
    t = torch.from_numpy(trip).cuda()
    d32, e32 = torch.empty(M_PUT, device="cuda"), torch.empty(M_PUT, device="cuda")
    nat.check(lib.dewi_payload_soa_f64(nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), nat.ptr(d32), nat.ptr(e32), M_PUT, nat.stream_ptr()))
    torch.cuda.synchronize()
    if normalize:
        assert bool(torch.isnan(e[11]).all())
    return x, t, e, h, d32, e32


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("dim", DIMS)
def test_rows_put_stores_the_bits_of_a_fresh_build(dim, base, normalize):
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    x, t, e_ref, h_ref, d_ref, en_ref = _put_reference(dim, normalize)
    big_e, E = _carve(CAP, dim, torch.float32, base)
    big_s, S = _carve(CAP, dim, torch.bfloat16, base)
    big_e.fill_(-7.0)
    big_s.fill_(-3.0)
    cols = torch.full((2, CAP + 4), -5.0, device="cuda")
    big_x, X = _carve(M_PUT, dim, torch.float32, base)           # the staging block at the same kind of address
    X.copy_(x)
    slots = np.random.RandomState(dim + 1).permutation(CAP)[:M_PUT].astype(np.int64)
    sl = torch.from_numpy(slots).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    before = [big_e.clone(), big_s.clone(), cols.clone()]
    nat.check(lib.dewi_rows_put_f32(E.data_ptr(), S.data_ptr(), cols[0].data_ptr(), cols[1].data_ptr(), CAP, dim, normalize,
                                    X.data_ptr(), nat.ptr(t[0]), nat.ptr(t[1]), nat.ptr(t[2]), nat.ptr(sl), M_PUT, nat.ptr(err),
                                    nat.stream_ptr()))
    assert int(err.item()) == 0
    assert np.array_equal(_i32(E[sl]), _i32(e_ref)), "stored rows"
    assert np.array_equal(_i16(S[sl]), _i16(h_ref)), "shadow rows"
    assert np.array_equal(_i32(cols[0, sl]), _i32(d_ref)) and np.array_equal(_i32(cols[1, sl]), _i32(en_ref)), "payload pair"
    # everything else — untouched slots, the bytes around the arrays — is as it was
    E[sl] = -7.0
    S[sl] = -3.0
    cols[:, sl] = -5.0
    for got, want, what in zip((big_e, big_s, cols), before, ("matrix", "shadow", "columns")):
        assert torch.equal(got, want), f"{what}: bytes outside the written slots changed"


def test_rows_put_without_a_shadow_and_with_slots_outside_the_capacity():
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    dim = 136
    x, t, e_ref, _, d_ref, _ = _put_reference(dim, 1)
    E = torch.full((CAP + 2, dim), -7.0, device="cuda")
    cols = torch.full((2, CAP + 2), -5.0, device="cuda")
    slots = np.arange(M_PUT, dtype=np.int64)
    slots[3], slots[20] = CAP, -1                                # one past the capacity (inside the allocation), one below 0
    sl = torch.from_numpy(slots).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    nat.check(lib.dewi_rows_put_f32(nat.ptr(E), 0, cols[0].data_ptr(), cols[1].data_ptr(), CAP, dim, 1, nat.ptr(x), nat.ptr(t[0]),
                                    nat.ptr(t[1]), nat.ptr(t[2]), nat.ptr(sl), M_PUT, nat.ptr(err), nat.stream_ptr()))
    assert int(err.item()) == 2
    good = np.flatnonzero((slots >= 0) & (slots < CAP))
    gi = torch.from_numpy(good).cuda()
    assert np.array_equal(_i32(E[gi]), _i32(e_ref[gi])) and np.array_equal(_i32(cols[0, gi]), _i32(d_ref[gi]))
    assert bool((E[[3, 20, CAP, CAP + 1]] == -7.0).all()) and bool((cols[:, [3, 20, CAP]] == -5.0).all())


# ---------------------------------------------------------------------------------------------------- index level
class _Docs:
    """The test's own dictionary id -> (raw row, Payload), and a generator of new documents."""

    def __init__(self, dim, seed):
        self.dim, self.rs, self.raw, self.pay, self.next = dim, np.random.RandomState(seed), {}, {}, 0

    def make(self, m):
        from dewi.types import Payload
        ids = [f"doc_{self.next + i:06d}" for i in range(m)]
        self.next += m
        raw = self.rs.standard_normal((m, self.dim)).astype(np.float32)
        vals = self.rs.rand(m, 4)
        pays = [Payload(dewi=float(v[0]), ht_mean=float(v[1]), hi_mean=float(v[2]), noise=float(v[3])) for v in vals]
        return ids, raw, pays

    def put(self, ids, raw, pays):
        for d, r, p in zip(ids, raw, pays):
            self.raw[d], self.pay[d] = np.array(r, dtype=np.float32), p

    def drop(self, ids):
        for d in ids:
            del self.raw[d], self.pay[d]

    @staticmethod
    def columns(pays):
        return {name: np.array([getattr(p, name) for p in pays]) for name in ("dewi", "ht_mean", "hi_mean", "noise")}


def _fresh(idx, docs, **kwargs):
    from dewi.backends import ExactIndex
    ids = list(idx._doc_ids)
    f = ExactIndex(idx.dim, idx.space, **kwargs)
    f.add_batch(ids, np.stack([docs.raw[d] for d in ids]), [docs.pay[d] for d in ids])
    f.build()
    return f


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def _same_as_fresh(idx, docs, Q, step, diverse, **kwargs):
    f = _fresh(idx, docs, **kwargs)
    a, b = idx._corpus, f._corpus
    assert a.n_rows == b.n_rows == len(idx._doc_ids) == len(docs.raw), step
    assert a.emb.is_contiguous() and a.capacity >= a.n_rows
    assert np.array_equal(_i32(a.emb), _i32(b.emb)), f"{step}: stored matrix"
    assert (a.shadow is None) == (b.shadow is None)
    if a.shadow is not None:
        assert np.array_equal(_i16(a.shadow), _i16(b.shadow)), f"{step}: shadow"
    assert np.array_equal(_i32(a.dewi32), _i32(b.dewi32)) and np.array_equal(_i32(a.ent32), _i32(b.ent32)), f"{step}: payload columns"
    for k in (1, 10, 64):
        got, want = idx.search_batch(Q, k, 0.3), f.search_batch(Q, k, 0.3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), f"{step}: search_batch k = {k}"
    thr = 0.25 if idx.space == "cosine" else -1.5 * idx.dim
    got, want = idx.range_search_batch(Q, thr, 0.3), f.range_search_batch(Q, thr, 0.3)
    assert int(want[0][-1]) > 0, "the range test needs rows above the threshold"
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want)), f"{step}: range_search_batch"
    dup_thr = 0.98 if idx.space == "cosine" else -0.05
    got, want = idx.duplicate_groups(dup_thr, keep="first"), f.duplicate_groups(dup_thr, keep="first")
    assert np.array_equal(got.labels, want.labels) and got.n_groups == want.n_groups, f"{step}: duplicate_groups"
    if diverse:
        got, want = idx.search_diverse_batch(Q, 10, 0.3), f.search_diverse_batch(Q, 10, 0.3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), f"{step}: search_diverse"
    d32, e32 = _i32(a.dewi32), _i32(a.ent32)
    idx.refresh_payloads()
    assert np.array_equal(_i32(a.dewi32), d32) and np.array_equal(_i32(a.ent32), e32), f"{step}: refresh_payloads"
    ids = list(idx._doc_ids)
    assert np.array_equal(idx.rows_of(ids), np.arange(len(ids))), f"{step}: rows_of"
    return f


def _ingest(idx, docs, n=1000):
    """Half as Payload objects, half as columns; one near-duplicate cluster (rows 400-407) and one zero embedding (row 650: it outlives every removal of the script)."""
    ids, raw, pays = docs.make(n)
    raw[401:408] = raw[400] + 1e-3 * docs.rs.standard_normal((7, docs.dim)).astype(np.float32)
    raw[ZERO_ROW] = 0.0
    h = n // 2
    idx.add_batch(ids[:h], raw[:h], pays[:h])
    idx.add_batch_columns(ids[h:], raw[h:], docs.columns(pays[h:]))
    docs.put(ids, raw, pays)
    idx.build()
    return ids


def _queries(docs, ids, dim):
    rs = np.random.RandomState(99)
    near = np.stack([docs.raw[ids[i]] for i in (400, 600, 700, 999)]) + 0.05 * rs.standard_normal((4, dim)).astype(np.float32)
    return np.concatenate([near, rs.standard_normal((4, dim)).astype(np.float32)]).astype(np.float32)


ZERO_ROW = 650
CONFIGS = [(50, "cosine", False), (132, "l2", False), (136, "cosine", True), (768, "cosine", True)]


@pytest.mark.parametrize("dim,space,shadow", CONFIGS, ids=[f"{d}-{s}{'-shadow' if b else ''}" for d, s, b in CONFIGS])
def test_a_mutated_index_equals_one_built_afresh(dim, space, shadow):
    """The script of the issue, and after every step the comparison with a fresh index.  Step 4 is split in two: 50 existing +
    200 new documents as the issue has it (698 + 200 rows stay below the capacity of 1 000, which never shrinks), then 250 more
    new ones, which do cross the capacity."""
    import torch
    from dewi.backends import ExactIndex
    kwargs = {"batch_shadow": True} if shadow else {}
    idx = ExactIndex(dim, space, **kwargs)
    docs = _Docs(dim, seed=dim)
    ids = _ingest(idx, docs)
    Q = _queries(docs, ids, dim)
    diverse = space == "cosine"
    keepers = {d: idx._payloads[d] for d in (ids[10], ids[450], ids[700], ids[990])}      # objects handed out: two per half

    def check(step):
        _same_as_fresh(idx, docs, Q, step, diverse, **kwargs)
        for d, p in keepers.items():
            if d in docs.raw:
                assert idx._payloads[d] is p and idx._payloads.get(d) is p, f"{step}: {d} got another Payload object"

    def remove(which, step):
        n0 = len(idx._doc_ids)
        want = mm.remove_ids(list(idx._doc_ids), which)
        assert idx.remove(which) == len(which)
        docs.drop(which)
        assert idx._doc_ids == want and len(idx._doc_ids) == n0 - len(which), f"{step}: row order"
        check(step)

    def upsert(known, m_new, step, how):
        new_ids, raw_n, pay_n = docs.make(m_new)
        _, raw_k, pay_k = docs.make(len(known))
        all_ids = list(known[: len(known) // 2]) + new_ids + list(known[len(known) // 2:])      # known and new ids interleaved
        raw = np.concatenate([raw_k[: len(known) // 2], raw_n, raw_k[len(known) // 2:]])
        pays = pay_k[: len(known) // 2] + pay_n + pay_k[len(known) // 2:]
        rows, want = mm.upsert_rows(list(idx._doc_ids), all_ids)
        if how == "objects":
            out = idx.upsert_batch(all_ids, raw, pays)
        elif how == "columns":
            out = idx.upsert_batch_columns(all_ids, raw, docs.columns(pays))
        else:                                                   # device-resident embeddings and dewi column
            cols = docs.columns(pays)
            cols["dewi"] = torch.from_numpy(cols["dewi"]).cuda()
            out = idx.upsert_batch_columns(all_ids, torch.from_numpy(raw).cuda(), cols)
        assert out == (len(known), m_new), step
        docs.put(all_ids, raw, pays)
        assert idx._doc_ids == want and idx.rows_of(all_ids).tolist() == rows, f"{step}: row order"
        check(step)

    assert idx.capacity == 1000
    check("as built")
    remove([ids[500]], "1: one middle document")
    remove([idx._doc_ids[-1]], "2: the last document")
    remove(list(idx._doc_ids[:300]), "3: the first 300")
    assert len(idx._doc_ids) == 698 and idx.capacity == 1000
    survivors = [d for d in idx._doc_ids if d != ids[ZERO_ROW] and d not in keepers]
    upsert(survivors[5:55], 200, "4a: 50 existing + 200 new", "objects")
    assert idx.capacity == 1000 and idx._corpus.reallocations == 0
    upsert([], 250, "4b: 250 new, across the capacity", "columns")
    assert len(idx._doc_ids) == 1148 and idx.capacity == max(1148, 1000 + 1000 // 4) and idx._corpus.reallocations == 1
    idx.reserve(2000)
    assert idx.capacity == 2000
    check("5: reserve")
    rs = np.random.RandomState(5)
    pool = [d for d in idx._doc_ids if d != ids[ZERO_ROW] and d not in keepers and d not in ids[400:408]]
    remove([pool[i] for i in rs.permutation(len(pool))[:600]], "6: 600 of 1148")
    for j in range(10):
        new_id, raw_1, pay_1 = docs.make(1)
        idx.upsert(new_id[0], raw_1[0], pay_1[0])
        docs.put(new_id, raw_1, pay_1)
        assert idx._doc_ids[-1] == new_id[0]
    assert idx._corpus.reallocations == 2 and idx.capacity == 2000            # (4b and the reserve)
    check("7: ten single upserts")
    assert ids[ZERO_ROW] in docs.raw
    other = next(d for d in idx._doc_ids if d != ids[ZERO_ROW] and d not in keepers)
    upsert([ids[ZERO_ROW], other], 1, "8: the zero embedding gets a real row", "device")
    assert not np.isnan(idx._embeddings[idx.rows_of([ids[ZERO_ROW]])[0]]).any()


def test_ten_single_appends_reallocate_at_most_once():
    from dewi.backends import ExactIndex
    docs = _Docs(50, seed=1)
    idx = ExactIndex(50, "cosine")
    ids, raw, pays = docs.make(200)
    idx.add_batch(ids, raw, pays)
    idx.build()
    assert idx.capacity == 200 and idx._corpus.reallocations == 0
    for _ in range(10):
        d, r, p = docs.make(1)
        idx.upsert(d[0], r[0], p[0])
    assert idx._corpus.reallocations <= 1 and len(idx._doc_ids) == 210 and idx.capacity >= 210


# ---------------------------------------------------------------------------------------------------- the shadow route
def test_the_shadow_route_after_remove_and_upsert():
    import torch
    from dewi.backends import ExactIndex
    n, dim = 65536, 136
    rs = np.random.RandomState(11)
    raw = rs.standard_normal((n, dim)).astype(np.float32)
    ids = [f"d{i}" for i in range(n)]
    cols = {"dewi": rs.rand(n), "ht_mean": rs.rand(n), "hi_mean": rs.rand(n)}
    idx = ExactIndex(dim, "cosine", batch_shadow=True)
    idx.add_batch_columns(ids, raw, cols)
    idx.build()
    gone = rs.choice(n, 1000, replace=False)
    assert idx.remove([ids[i] for i in gone.tolist()]) == 1000
    keep = np.setdiff1d(np.arange(n), gone)
    up_old = rs.choice(keep, 500, replace=False)                       # 500 replaced, 1 000 new: 65 536 rows again
    up_ids = [ids[i] for i in up_old.tolist()] + [f"new{i}" for i in range(1000)]
    up_raw = rs.standard_normal((1500, dim)).astype(np.float32)
    up_cols = {name: rs.rand(1500) for name in cols}
    assert idx.upsert_batch_columns(up_ids, up_raw, up_cols) == (500, 1000)
    assert len(idx._doc_ids) == n
    # the same documents, afresh, in the mutated order
    raw_of = {d: raw[i] for i, d in enumerate(ids)}
    col_of = {d: tuple(cols[name][i] for name in cols) for i, d in enumerate(ids)}
    for j, d in enumerate(up_ids):
        raw_of[d], col_of[d] = up_raw[j], tuple(up_cols[name][j] for name in cols)
    order = list(idx._doc_ids)
    f = ExactIndex(dim, "cosine", batch_shadow=True)
    f.add_batch_columns(order, np.stack([raw_of[d] for d in order]),
                        {name: np.array([col_of[d][c] for d in order]) for c, name in enumerate(cols)})
    f.build()
    assert np.array_equal(_i32(idx._corpus.emb), _i32(f._corpus.emb)) and np.array_equal(_i16(idx._corpus.shadow), _i16(f._corpus.shadow))
    Q = np.concatenate([up_raw[:16] + 0.1 * rs.standard_normal((16, dim)).astype(np.float32), rs.standard_normal((16, dim)).astype(np.float32)])
    got, want = idx.search_batch(Q, 10, 0.3), f.search_batch(Q, 10, 0.3)
    assert idx._corpus._last_call[3] is True, "the batch must have gone through the shadow"
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    c = idx._corpus
    with torch.cuda.device(c.device):
        # without the shadow: the one-query search over the fp32 rows, which the shadow route equals bit for bit (a BATCH
        # without the shadow takes the fp32 matrix-core pass, whose sums are ordered differently: not the contract)
        q_dev = c.stage_queries(Q).clone()
        for j in range(Q.shape[0]):
            ids_d, sc_d = c.search_device(q_dev[j:j + 1], 10, 0.3, 0.0, use_shadow=False)
            assert c._last_call[3] is False
            assert np.array_equal(ids_d.cpu().numpy()[0], got[0][j]) and np.array_equal(_bits(sc_d.cpu().numpy()[0]), _bits(got[1][j])), j


# ---------------------------------------------------------------------------------------------------- filters
def _small_index(dim=50, n=400, seed=2, cls=None, **kwargs):
    from dewi.backends import ExactIndex
    docs = _Docs(dim, seed=seed)
    idx = (cls or ExactIndex)(dim, "cosine", **kwargs)
    ids, raw, pays = docs.make(n)
    idx.add_batch(ids, raw, pays)
    docs.put(ids, raw, pays)
    idx.build()
    return idx, docs, ids


@pytest.mark.parametrize("mutation", ["remove", "upsert"])
def test_filters_made_before_a_mutation_are_refused_and_remade_ones_answer_like_the_fresh_index(mutation):
    idx, docs, ids = _small_index()
    Q = np.random.RandomState(0).standard_normal((4, 50)).astype(np.float32)
    allowed = ids[50:250]
    masks = np.random.RandomState(1).rand(4, 400) < 0.5
    flt, qf = idx.make_filter(doc_ids=allowed), idx.make_query_filters(masks)
    idx.search_batch(Q, 5, 0.3, filter=flt), idx.search_batch(Q, 5, 0.3, filter=qf)
    if mutation == "remove":
        gone = ids[100:120] + ids[300:310]
        idx.remove(gone)
        docs.drop(gone)
    else:
        d, r, p = docs.make(1)
        idx.upsert(ids[7], r[0], p[0])
        docs.put([ids[7]], r, p)
    with pytest.raises(ValueError, match="this filter was prepared for another corpus"):
        idx.search_batch(Q, 5, 0.3, filter=flt)
    with pytest.raises(ValueError, match="these query filters were prepared for another corpus"):
        idx.search_batch(Q, 5, 0.3, filter=qf)
    with pytest.raises(ValueError, match="this filter was prepared for another corpus"):
        idx.range_search_batch(Q, 0.2, 0.3, filter=flt)
    f = _fresh(idx, docs)
    allowed = [d for d in allowed if d in docs.raw]
    got, want = idx.search_batch(Q, 5, 0.3, filter=idx.make_filter(doc_ids=allowed)), f.search_batch(Q, 5, 0.3, filter=f.make_filter(doc_ids=allowed))
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    m2 = masks[:, : len(idx._doc_ids)]
    got, want = idx.search_batch(Q, 5, 0.3, filter=idx.make_query_filters(m2)), f.search_batch(Q, 5, 0.3, filter=f.make_query_filters(m2))
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_dedup_filter_picks_the_next_representative_once_the_first_is_removed():
    from dewi.backends import ExactIndex
    from dewi.types import Payload
    dim, n = 50, 300
    rs = np.random.RandomState(4)
    raw = rs.standard_normal((n, dim)).astype(np.float32)
    raw[201:205] = raw[200] + 1e-4 * rs.standard_normal((4, dim)).astype(np.float32)         # one cluster: rows 200-204
    dewi = rs.rand(n) * 0.5
    dewi[202], dewi[204] = 0.9, 0.8                                                           # its best, and its second best
    ids = [f"d{i}" for i in range(n)]
    idx = ExactIndex(dim, "cosine")
    idx.add_batch(ids, raw, [Payload(dewi=float(v)) for v in dewi])
    idx.build()
    q = raw[200:201]

    def kept(flt):
        rows, _ = idx.search_batch(q, 5, 0.0, filter=flt)
        return [idx._doc_ids[r] for r in rows[0].tolist() if idx._doc_ids[r] in ids[200:205]]

    assert kept(idx.dedup_filter(0.99, keep="dewi")) == ["d202"]
    assert idx.remove(["d202"]) == 1
    assert kept(idx.dedup_filter(0.99, keep="dewi")) == ["d204"]
    groups = idx.duplicate_groups(0.99, keep="dewi", doc_ids=True)
    assert sorted(max(groups.clusters, key=len)) == ["d200", "d201", "d203", "d204"]


# ---------------------------------------------------------------------------------------------------- IVFIndex
def test_ivf_cells_follow_the_rows_without_retraining():
    from dewi.ivf import IVFIndex
    n, dim, nlist = 4096, 64, 16
    idx, docs, ids = _small_index(dim, n, seed=6, cls=IVFIndex, nlist=nlist, train_seed=3)
    cent0, cells0 = idx.centroids.copy(), idx.cell_of_row.copy()
    rs = np.random.RandomState(8)
    gone = [ids[i] for i in rs.choice(n, 500, replace=False).tolist()]
    order = mm.remove_order(n, idx.rows_of(gone).tolist())
    assert idx.remove(gone) == 500
    docs.drop(gone)
    assert np.array_equal(_bits(idx.centroids), _bits(cent0)), "the centroids were touched"
    cells1 = idx.cell_of_row
    assert cells1.shape == (n - 500,) and np.array_equal(cells1, cells0[order]), "a survivor changed its cell"
    # upserts planted next to a centroid land in its cell: 100 existing documents and 60 new ones
    up_ids = [d for d in idx._doc_ids[::30]][:100]
    new_ids, _, new_pays = docs.make(60)
    _, _, old_pays = docs.make(100)
    all_ids, pays = up_ids + new_ids, old_pays + new_pays
    want_cell = rs.randint(0, nlist, len(all_ids))
    raw = (cent0[want_cell] + 1e-3 * rs.standard_normal((len(all_ids), dim))).astype(np.float32)
    rows, _ = mm.upsert_rows(list(idx._doc_ids), all_ids)
    assert idx.upsert_batch(all_ids, raw, pays) == (100, 60)
    docs.put(all_ids, raw, pays)
    cells2 = idx.cell_of_row
    assert np.array_equal(_bits(idx.centroids), _bits(cent0))
    assert cells2.shape == (n - 440,) and np.array_equal(cells2[rows], want_cell), "a planted row missed its cell"
    untouched = np.setdiff1d(np.arange(n - 500), rows)
    assert np.array_equal(cells2[untouched], cells1[untouched])
    offsets, listed, G = idx.cell_lists()
    m_off, m_rows, dropped = ivf_model.lists_model(cells2, nlist, G)
    assert dropped == 0 and np.array_equal(offsets, m_off) and np.array_equal(listed, m_rows)
    assert idx._ivf.corpus_id == idx._corpus.corpus_id
    f = _fresh(idx, docs)
    Q = np.concatenate([raw[:4], rs.standard_normal((4, dim)).astype(np.float32)])
    got, want = idx.search_batch(Q, 10, 0.3, nprobe=nlist), f.search_batch(Q, 10, 0.3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(_bits(idx.centroids), _bits(cent0)), "a search after the mutation retrained"
    with pytest.raises(ValueError, match="the index has 16 cells"):
        idx.remove(list(idx._doc_ids[: len(idx._doc_ids) - 10]))
    assert len(idx._doc_ids) == n - 440


# ---------------------------------------------------------------------------------------------------- DewiIndex
def test_dewi_index_remove_upsert_accessors_and_persistence(tmp_path):
    from dewi.index import DewiIndex
    dim = 50
    docs = _Docs(dim, seed=9)
    idx = DewiIndex(dim=dim, use_ann=False, rerank_eta=0.3)
    ids, raw, pays = docs.make(200)
    for d, r, p in zip(ids[:20], raw[:20], pays[:20]):
        idx.add(d, r, p, meta={"n": d})
    idx.add_batch(ids[20:], raw[20:], pays[20:])
    idx.build()
    assert idx.remove([ids[3], ids[100]]) == 2 and len(idx) == 198
    for d in (ids[3], ids[100]):
        assert idx.get_payload(d) is None and idx.get_embedding(d) is None and idx.get_metadata(d) is None
    assert idx.get_metadata(ids[4]) == {"n": ids[4]} and idx.get_payload(ids[199]) is pays[199]
    new_id, new_raw, new_pay = docs.make(1)
    idx.upsert(new_id[0], new_raw[0], new_pay[0], meta={"fresh": True})
    idx.upsert(ids[5], new_raw[0] * 2, new_pay[0])
    assert len(idx) == 199 and idx.get_metadata(new_id[0]) == {"fresh": True} and idx.get_metadata(ids[5]) == {"n": ids[5]}
    assert idx.get_payload(new_id[0]) is new_pay[0] and idx.rows_of([new_id[0]]).tolist() == [198]
    unit = new_raw[0] / np.linalg.norm(new_raw[0])
    assert np.allclose(idx.get_embedding(new_id[0]), unit, atol=1e-6) and np.allclose(idx.get_embedding(ids[5]), unit, atol=1e-6)
    assert idx.search(new_raw[0], k=2)[0][0] in (new_id[0], ids[5])
    Q = np.random.RandomState(1).standard_normal((5, dim)).astype(np.float32)
    before = idx.search_batch(Q, k=7)
    idx.save(tmp_path / "ix")
    back = DewiIndex.load(tmp_path / "ix")
    assert back._backend._doc_ids == idx._backend._doc_ids and back.get_metadata(ids[3]) is None
    after = back.search_batch(Q, k=7)
    assert [[(d, s) for d, s, _ in row] for row in after] == [[(d, s) for d, s, _ in row] for row in before]


# ---------------------------------------------------------------------------------------------------- errors
def test_a_failing_call_leaves_the_index_as_it_was():
    from dewi.types import Payload
    idx, docs, ids = _small_index(50, 100, seed=12)
    Q = np.random.RandomState(2).standard_normal((3, 50)).astype(np.float32)
    before = idx.search_batch(Q, 5, 0.3)
    flt = idx.make_filter(doc_ids=ids[:50])
    good = np.ones((2, 50), np.float32)
    p = [Payload(), Payload()]
    calls = [
        (KeyError, "unknown doc ids", lambda: idx.remove([ids[0], "nobody"])),
        (ValueError, "must be distinct", lambda: idx.remove([ids[0], ids[1], ids[0]])),
        (ValueError, "cannot remove every document", lambda: idx.remove(list(ids))),
        (ValueError, "must be distinct", lambda: idx.upsert_batch(["a", "a"], good, p)),
        (ValueError, r"Expected embeddings of shape \(m, 50\), got \(2, 49\)", lambda: idx.upsert_batch(["a", "b"], good[:, :49], p)),
        (ValueError, "must have the same length", lambda: idx.upsert_batch(["a"], good, p)),
        (ValueError, r"Expected embedding of shape \(50,\), got \(49,\)", lambda: idx.upsert("a", good[0, :49], p[0])),
        (ValueError, r"Expected embeddings of shape \(m, 50\)", lambda: idx.upsert_batch_columns(["a", "b"], good[:, :49], {})),
        (ValueError, "unknown payload columns", lambda: idx.upsert_batch_columns(["a", "b"], good, {"nope": np.zeros(2)})),
        (ValueError, "payload column 'dewi' has shape", lambda: idx.upsert_batch_columns(["a", "b"], good, {"dewi": np.zeros(3)})),
        (KeyError, "unknown doc ids", lambda: idx.rows_of(["nobody"])),
    ]
    for exc, message, call in calls:
        with pytest.raises(exc, match=message):
            call()
        assert len(idx._doc_ids) == 100 and idx._doc_ids == ids and "a" not in idx._payloads
        after = idx.search_batch(Q, 5, 0.3)
        assert np.array_equal(after[0], before[0]) and np.array_equal(_bits(after[1]), _bits(before[1]))
        idx.search_batch(Q, 5, 0.3, filter=flt)                   # nothing happened: the filter is still this corpus's
    assert idx.remove([]) == 0 and idx.upsert_batch([], np.zeros((0, 50), np.float32), []) == (0, 0)
    idx.search_batch(Q, 5, 0.3, filter=flt)


def test_an_index_that_holds_an_id_twice_cannot_be_mutated_by_id():
    from dewi.backends import ExactIndex
    docs = _Docs(50, seed=13)
    ids, raw, pays = docs.make(20)
    idx = ExactIndex(50, "cosine")
    idx.add_batch(ids + [ids[4]], np.concatenate([raw, raw[:1]]), pays + pays[:1])
    idx.build()
    for call in (lambda: idx.remove([ids[0]]), lambda: idx.upsert(ids[4], raw[0], pays[0]), lambda: idx.rows_of([ids[1]])):
        with pytest.raises(ValueError, match="holds doc ids more than once"):
            call()
    assert len(idx._doc_ids) == 21


def test_a_bf16_main_matrix_is_not_mutable():
    idx, _, _ = _small_index(136, 100, seed=14)
    half = idx._corpus.to_bf16()
    one = np.ones((1, 136), np.float32)
    with pytest.raises(NotImplementedError, match="bf16 main matrix"):
        half.remove_rows([3])
    with pytest.raises(NotImplementedError, match="bf16 main matrix"):
        half.put_rows([3], one, [0.0], [0.0], [0.0])
    with pytest.raises(NotImplementedError, match="bf16 main matrix"):
        half.reserve(1000)
    assert half.n_rows == 100


def test_corpus_level_argument_checks():
    from dewi._engine import plan_remove
    idx, _, _ = _small_index(50, 100, seed=15)
    c = idx._corpus
    cid = c.corpus_id
    one = np.ones((2, 50), np.float32)
    z = [0.0, 0.0]
    for rows in ([100, 102], [5, 5], [-1, 3], [101]):
        with pytest.raises(ValueError, match="rows to put must be distinct rows"):
            c.put_rows(rows, one[: len(rows)], z[: len(rows)], z[: len(rows)], z[: len(rows)])
    with pytest.raises(ValueError, match=r"Expected embeddings of shape \(2, 50\)"):
        c.put_rows([1, 2], one[:, :40], z, z, z)
    with pytest.raises(ValueError, match="one value per row"):
        c.put_rows([1, 2], one, [0.0], z, z)
    with pytest.raises(ValueError, match="rows to remove must be distinct"):
        c.remove_rows([1, 1])
    assert c.corpus_id == cid and c.n_rows == 100
    src, dst = c.remove_rows([0, 99])
    assert (src.tolist(), dst.tolist()) == tuple(x.tolist() for x in plan_remove(100, [0, 99])[:2]) == ([98], [0])
    assert c.n_rows == 98 and c.corpus_id != cid and not c.cached_workspaces() and c._last_call is None

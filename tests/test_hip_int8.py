"""GPU: the approximate route over an int8 copy of the corpus (csrc/knn_scan_i8.hip) against tests/int8_model.py.

The int8 arithmetic is integer, so everything up to the candidate records is compared BIT FOR BIT: the codes and scales of the
stored rows, the prepared queries (the norm is a float64 sum in another order: scales within 1 ulp, codes within one step —
from there on the model is fed the library's own prepared form), the records (ids, sim bits, order, padding).  The re-scoring
is fp32 in a fixed order: bit for bit where every order gives the same sum, within the accumulation bound otherwise.

Shapes are the smallest that reach every path: both geometries (rows of 1 .. 32 and of 33 .. 256 units of 16 codes), every
units-per-lane count and rows-in-flight choice, masked lanes (rows that are no multiple of 64 units), tails shorter than the rows
in flight, more than one workgroup, the three list forms (c <= 64, c <= 256, dense) and passes of four queries plus a remainder.
"""
import numpy as np
import pytest

import diverse_model as dm
import int8_model as im
import rerank_model as rm
import wsguard

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
_cache = {}


def _lib():
    from dewi import _native as nat
    return nat.load_library()


def unit_rows(n, dim, seed):
    x = np.random.RandomState(seed).randn(n, dim)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def payload(n, seed):
    rs = np.random.RandomState(seed + 77)
    return rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)


def quantize_dev(E_dev):
    """``dewi_quantize_rows_i8`` -> (codes int8 [n, dim], scales fp32 [n]) device tensors."""
    import torch
    from dewi import _native as nat
    n, dim = int(E_dev.shape[0]), int(E_dev.shape[1])
    codes = torch.empty((n, dim), dtype=torch.int8, device="cuda")
    scales = torch.empty(n, dtype=torch.float32, device="cuda")
    nat.check(_lib().dewi_quantize_rows_i8(nat.ptr(E_dev), n, dim, nat.ptr(codes), nat.ptr(scales), nat.stream_ptr()))
    return codes, scales


def prepare_dev(Q_dev):
    """``dewi_prepare_queries_i8`` -> host (codes int8 [B, dim], scales fp32 [B], normalised queries fp32 [B, dim])."""
    import torch
    from dewi import _native as nat
    b, dim = int(Q_dev.shape[0]), int(Q_dev.shape[1])
    codes = torch.empty((b, dim), dtype=torch.int8, device="cuda")
    scales = torch.empty(b, dtype=torch.float32, device="cuda")
    qn = torch.empty((b, dim), dtype=torch.float32, device="cuda")
    nat.check(_lib().dewi_prepare_queries_i8(nat.ptr(Q_dev), b, dim, nat.ptr(codes), nat.ptr(scales), nat.ptr(qn), nat.stream_ptr()))
    torch.cuda.synchronize()
    return codes.cpu().numpy(), scales.cpu().numpy(), qn.cpu().numpy()


def candidates_dev(codes, scales, Q_dev, dewi_dev, ent_dev, c, id_offset=0):
    """``dewi_knn_candidates_i8`` in a workspace of exactly the required size -> records [B, c] on the host."""
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    lib = _lib()
    n, dim, b = int(codes.shape[0]), int(codes.shape[1]), int(Q_dev.shape[0])
    need = int(lib.dewi_knn_i8_workspace_bytes(n, dim, b, c))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((b, c, 4), dtype=torch.int32, device="cuda")
    nat.check(lib.dewi_knn_candidates_i8(nat.ptr(codes), nat.ptr(scales), n, dim, nat.ptr(Q_dev), b, nat.ptr(dewi_dev), nat.ptr(ent_dev),
                                         c, id_offset, nat.ptr(out), nat.ptr(ws), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    return records_to_numpy(out)


def rescore_dev(E_dev, Q_dev, recs, id_offset=0):
    import torch
    from dewi import _native as nat
    from dewi._engine import records_to_numpy
    b, c = recs.shape
    d = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(b, c, 4)).cuda()
    nat.check(_lib().dewi_rescore_candidates_f32(nat.ptr(E_dev), int(E_dev.shape[0]), int(E_dev.shape[1]), nat.ptr(Q_dev), b, nat.ptr(d),
                                                 c, id_offset, nat.stream_ptr()))
    torch.cuda.synchronize()
    return records_to_numpy(d)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def assert_records_equal(got, want, what):
    for name in ("id", "sim", "dewi", "ent"):
        if not same_bits(got[name], want[name]):
            bad = np.argwhere(np.ascontiguousarray(got[name]).view(np.uint32) != np.ascontiguousarray(want[name]).view(np.uint32))
            q, t = bad[0]
            raise AssertionError(f"{what}: field {name} differs at query {q} position {t} ({bad.shape[0]} places): "
                                 f"got {got[q, t]} want {want[q, t]}")


# ------------------------------------------------------------------------------------------------------------ quantise
def planted_rows(n, dim, seed):
    """Gaussian unit rows with, from 63 rows on: a NaN element, an inf element, a zero row, a row with elements exactly on a
    .5 code boundary (scale 1 / 128) and a flat +-max row."""
    x = unit_rows(n, dim, seed)
    if n >= 63:
        x[3, dim // 2] = np.nan
        x[9, dim - 1] = -np.inf
        x[17] = 0
        x[25] = 0
        x[25, 0], x[25, 1], x[25, 2], x[25, dim - 1] = 127 / 128, 2.5 / 128, 3.5 / 128, -0.5 / 128
        x[40] = np.float32(0.25) * np.where(np.arange(dim) % 3 == 0, -1, 1)
    return x


@pytest.mark.parametrize("n", [1, 63, 1000])
@pytest.mark.parametrize("dim", [16, 48, 512, 528, 768, 1024, 1040, 4096])
def test_quantised_rows_equal_the_model(dim, n):
    import torch
    from dewi._engine import DeviceCorpus
    x = planted_rows(n, dim, dim + n)
    z = np.zeros(n)
    corpus = DeviceCorpus.from_host(x, z, z, z, "cosine", normalize=False)
    corpus.enable_int8_shadow()
    torch.cuda.synchronize()
    stored = corpus.emb.cpu().numpy()
    assert same_bits(stored, x)
    codes, scales = im.quantize(stored)
    assert same_bits(corpus.i8_scales.cpu().numpy(), scales), "scales"
    assert np.array_equal(corpus.i8_codes.cpu().numpy(), codes), "codes"
    if n >= 63:
        assert np.isnan(scales[[3, 9]]).all() and scales[17] == 0 and scales[25] == np.float32(1 / 128)
        assert codes[25, :3].tolist() == [127, 2, 4] and codes[25, dim - 1] == 0 and (np.abs(codes[40]) == 127).all()


# ------------------------------------------------------------------------------------------------------------ queries
@pytest.mark.parametrize("dim", [16, 48, 512, 528, 1040, 4096])
def test_prepared_queries(dim):
    import torch
    q = (np.random.RandomState(dim).randn(7, dim) * 3).astype(np.float32)
    q[2] = 0
    q[4, dim // 3] = np.nan
    q[5, 1] = np.inf
    codes, scales, qn = prepare_dev(torch.from_numpy(q).cuda())
    mc, ms, mqn = im.prepare_query(q)
    fin = [0, 1, 3, 6]
    ulp = np.abs(scales[fin].view(np.int32).astype(np.int64) - ms[fin].view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp
    step = np.abs(codes[fin].astype(np.int32) - mc[fin].astype(np.int32))
    assert step.max() <= 1 and (step == 0).mean() >= 0.99
    assert np.allclose(qn[fin], mqn[fin], rtol=3e-7, atol=0)
    # a zero query, a NaN query and an inf query are the model's bit for bit
    for j in (2, 4, 5):
        assert same_bits(scales[j], ms[j]) and np.array_equal(codes[j], mc[j]), j
    assert same_bits(qn[2], q[2]) and same_bits(qn[4], q[4])
    # the codes are Q of the library's own normalised query, bit for bit
    own_c, own_s = im.quantize(qn)
    assert np.array_equal(own_c, codes) and same_bits(own_s, scales)


# ------------------------------------------------------------------------------------------------------------ candidates
def corpus_rows(kind, n, dim, seed):
    if kind == "gauss":
        return unit_rows(n, dim, seed)
    if kind == "flat":           # +-1 / sqrt(dim), exact at dim 4096: |D| reaches 127^2 * 4096 > 2^24
        rs = np.random.RandomState(seed)
        x = (rs.choice(np.array([-1.0, 1.0]), (n, dim)) / np.sqrt(dim)).astype(np.float32)
        x[n // 2] = x[0]
        x[n // 3] = -x[0]
        return x
    assert kind == "ties"        # 40 identical rows, NaN rows, a zero row
    x = unit_rows(n, dim, seed)
    x[100:140] = x[5]
    x[7, 3] = np.nan
    x[n - 1, 0] = np.nan
    x[300] = 0
    return x


# (dim, n, c, B, corpus, id_offset): every value of every axis of the issue's grid, and every (units per lane, rows in flight)
CANDIDATE_CASES = [
    (16, 1, 1, 1, "gauss", 0), (16, 1, 4, 3, "gauss", 5), (16, 4099, 64, 4, "gauss", 7), (48, 1000, 65, 3, "gauss", 0),
    (48, 63, 256, 5, "gauss", 0), (512, 4099, 256, 5, "gauss", 0), (512, 1000, 257, 1, "gauss", 0),
    (528, 1000, 257, 4, "gauss", 1000), (528, 4099, 1, 1, "gauss", 0), (768, 4099, 20, 1, "gauss", 0),
    (768, 4099, 1024, 4, "gauss", 0), (768, 1000, 50, 3, "ties", 11), (768, 1000, 100, 5, "ties", 0),
    (1024, 63, 100, 1, "gauss", 0), (1024, 1000, 64, 5, "gauss", 0), (1040, 1000, 10, 5, "gauss", 0),
    (1040, 4099, 65, 1, "gauss", 3), (4096, 1000, 64, 1, "flat", 0), (4096, 63, 1, 4, "flat", 0), (4096, 1000, 300, 3, "gauss", 0),
    (1280, 1000, 10, 1, "gauss", 0), (1536, 1000, 70, 4, "gauss", 0), (2064, 1000, 10, 5, "gauss", 0), (3104, 63, 10, 4, "gauss", 0),
    (3104, 1000, 300, 1, "gauss", 0), (256, 1000, 10, 1, "ties", 0), (32, 4099, 100, 5, "gauss", 0),
]


@pytest.mark.parametrize("dim,n,c,b,kind,id_offset", CANDIDATE_CASES)
def test_candidate_records_equal_the_model(dim, n, c, b, kind, id_offset):
    import torch
    x = corpus_rows(kind, n, dim, 31 * dim + n)
    q = (np.random.RandomState(c + b).randn(b, dim)).astype(np.float32)
    q[0] = x[0] if kind != "ties" else x[5]
    dewi, ent = payload(n, dim)
    E_dev, Q_dev = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    codes, scales = quantize_dev(E_dev)
    got = candidates_dev(codes, scales, Q_dev, torch.from_numpy(dewi).cuda(), torch.from_numpy(ent).cuda(), c, id_offset)
    qc, qs, _ = prepare_dev(Q_dev)
    rc, rsc = codes.cpu().numpy(), scales.cpu().numpy()
    want = im.candidates(rc, rsc, qc, qs, dewi, ent, c, id_offset)
    assert_records_equal(got, want, f"{dim} x {n}, c {c}, B {b}, {kind}")
    if kind == "flat":
        d = rc.astype(np.int64) @ qc[0].astype(np.int64)
        assert np.abs(d).max() == 127 * 127 * dim > 2 ** 24
    if kind == "ties":
        first = got["id"][0] - id_offset
        assert np.isnan(got["sim"][0, :2]).all() and sorted(first[:2].tolist()) == [7, n - 1]
        m = min(c - 2, 41)
        assert first[2:2 + m].tolist() == ([5] + list(range(100, 140)))[:m]
    if c > n:
        assert (got["id"][:, n:] == -1).all() and np.isneginf(got["sim"][:, n:]).all()


# ------------------------------------------------------------------------------------------------------------ rescore
def dyadic_rows(n, dim, seed):
    """Entries k / 64 with |k| <= 8: with a query of +-0.25 in 16 places every partial sum is a multiple of 1 / 256 below 1."""
    return (np.random.RandomState(seed).randint(-8, 9, (n, dim)) / 64.0).astype(np.float32)


def dyadic_queries(b, dim, seed):
    """16 entries of +-0.5: norm exactly 2, the normalised query +-0.25."""
    rs = np.random.RandomState(seed)
    q = np.zeros((b, dim), np.float32)
    for j in range(b):
        q[j, rs.choice(dim, 16, replace=False)] = rs.choice(np.array([0.5, -0.5], np.float32), 16)
    return q


def arbitrary_records(rs, b, c, n, id_offset):
    recs = np.zeros((b, c), rm.RECORD)
    for j in range(b):
        recs["sim"][j] = rs.choice(np.array([0.5, 0.25, -0.0, 7.0, -3.0], np.float32), c)
        recs["dewi"][j] = rs.rand(c).astype(np.float32)
        recs["ent"][j] = rs.rand(c).astype(np.float32)
        assert c <= n                       # distinct ids: two records with one (sim, id) have no order
        recs["id"][j] = rs.permutation(n)[:c] + id_offset
        bad = np.nonzero(rs.rand(c) < 0.1)[0]
        recs["id"][j][bad] = id_offset + n + np.arange(bad.shape[0])        # ids that are no row: behind the rows, ...
        if bad.shape[0] > 0:
            recs["id"][j][bad[0]] = 2 ** 31 - 1
        if bad.shape[0] > 1 and id_offset:
            recs["id"][j][bad[1]] = id_offset - 1                           # ... and in front of them
        n_valid = c if j % 2 == 0 else int(rs.randint(0, c + 1))
        recs[j, n_valid:] = (-np.inf, 0.0, 0.0, -1)
        if c >= 8 and j % 3 == 0:          # padding in the middle too: it goes behind the records in its old order
            recs[j, 2] = (-np.inf, 0.0, 0.0, -1)
            recs[j, 5] = (1.5, 1.0, 2.0, -2)
    return recs


@pytest.mark.parametrize("dim,n,c,b,id_offset", [(16, 40, 1, 1, 0), (16, 100, 64, 3, 9), (768, 200, 20, 1, 0), (768, 300, 257, 5, 1000),
                                                  (1040, 120, 100, 2, 0), (4096, 1100, 1024, 2, 0), (48, 90, 65, 4, 0)])
def test_rescore_is_exact_on_dyadic_rows(dim, n, c, b, id_offset):
    import torch
    rs = np.random.RandomState(dim + c)
    x, q = dyadic_rows(n, dim, dim), dyadic_queries(b, dim, c)
    Q_dev = torch.from_numpy(q).cuda()
    _, _, qn = prepare_dev(Q_dev)
    assert same_bits(qn, q / np.float32(2))
    recs = arbitrary_records(rs, b, c, n, id_offset)
    got = rescore_dev(torch.from_numpy(x).cuda(), Q_dev, recs, id_offset)
    want = im.rescore(recs, x, qn, id_offset)
    assert_records_equal(got, want, f"rescore {dim} x {n}, c {c}, B {b}")
    for j in range(b):
        local = recs["id"][j].astype(np.int64) - id_offset
        out_of_range = (recs["id"][j] >= 0) & ((local < 0) | (local >= n))
        after = {got[j, u].tobytes() for u in range(c)}
        for t in np.nonzero(out_of_range | (recs["id"][j] < 0))[0]:
            assert recs[j, t].tobytes() in after, "a record that is no row was changed"


@pytest.mark.parametrize("dim", [16, 768, 4096])
def test_rescore_on_unit_rows_within_the_accumulation_bound(dim):
    import torch
    n, c, b = 500, 200, 4
    x = unit_rows(n, dim, dim)
    x[7, 1] = np.nan
    q = np.random.RandomState(9).randn(b, dim).astype(np.float32) * 4
    E_dev, Q_dev = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    dewi, ent = payload(n, dim)
    codes, scales = quantize_dev(E_dev)
    recs = candidates_dev(codes, scales, Q_dev, torch.from_numpy(dewi).cuda(), torch.from_numpy(ent).cuda(), c, 3)
    got = rescore_dev(E_dev, Q_dev, recs, 3)
    _, _, qn = prepare_dev(Q_dev)
    for j in range(b):
        assert sorted(got["id"][j].tolist()) == sorted(recs["id"][j].tolist())
        rows = got["id"][j].astype(np.int64) - 3
        ref = x[rows].astype(np.float64) @ qn[j].astype(np.float64)
        assert got["id"][j, 0] == 7 + 3 and np.isnan(got["sim"][j, 0]), "the NaN row stays first"
        err = np.abs(got["sim"][j, 1:].astype(np.float64) - ref[1:])
        assert err.max() <= dim * EPS * 1.0002, (err.max(), dim * EPS)
        assert np.array_equal(rm.record_order(got[j]), np.arange(c)), "sorted again by (ord(sim) desc, id asc)"
        keep = {int(r["id"]): (r["dewi"], r["ent"]) for r in recs[j]}
        assert all(keep[int(r["id"])] == (r["dewi"], r["ent"]) for r in got[j])


# ------------------------------------------------------------------------------------------------------------ end to end
def columns(n, seed):
    rs = np.random.RandomState(seed)
    return {"dewi": rs.rand(n), "ht_mean": rs.rand(n), "hi_mean": rs.rand(n)}


def build_index(x, cols, cls="exact", **kwargs):
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    ids = [f"d{i:06d}" for i in range(x.shape[0])]
    idx = ExactIndex(x.shape[1], **kwargs) if cls == "exact" else DewiIndex(x.shape[1], use_ann=False, **kwargs)
    idx.add_batch_columns(ids, x, cols)
    idx.build()
    return idx


def shadowed(dim):
    """(raw rows, payload columns, queries, an ExactIndex with an int8 shadow) — built once per dim."""
    if ("idx", dim) not in _cache:
        n = 3000
        x = np.random.RandomState(dim).randn(n, dim).astype(np.float32)
        x[50:60] = x[49]
        cols = columns(n, dim)
        q = np.random.RandomState(dim + 1).randn(6, dim).astype(np.float32)
        q[1] = x[49]
        _cache[("idx", dim)] = (x, cols, q, build_index(x, cols, int8_shadow=True))
    return _cache[("idx", dim)]


def model_records(idx, q, c):
    """The model's records of an index: from its stored rows' codes (the library's, checked above) and the library's prepared queries."""
    import torch
    corpus = idx._corpus
    codes, scales = corpus._int8()
    qc, qs, qn = prepare_dev(torch.from_numpy(q).cuda())
    recs = im.candidates(codes.cpu().numpy(), scales.cpu().numpy(), qc, qs, corpus.dewi32.cpu().numpy(), corpus.ent32.cpu().numpy(), c)
    return recs, qn


@pytest.mark.parametrize("dim", [128, 768])
@pytest.mark.parametrize("eta,pref", [(0.0, 0.0), (0.3, 0.0), (0.3, 0.2), (0.0, 0.2)])
def test_search_without_rescore_equals_the_model(dim, eta, pref):
    x, cols, q, idx = shadowed(dim)
    for k, cand in ((10, None), (7, 100), (150, None)):
        c = min(2 * k, x.shape[0]) if cand is None else cand
        rows, scores = idx.search_batch(q, k, eta, pref, cand, approx=True, rescore=False)
        recs, _ = model_records(idx, q, c)
        want_ids, want_sc = im.search(recs, k, eta, pref)
        assert np.array_equal(rows, want_ids), (k, cand)
        assert same_bits(scores, want_sc), (k, cand)
    # the facade and one query
    one = idx.search(q[1], 5, eta, pref, approx=True, rescore=False)
    recs, _ = model_records(idx, q[1:2], 10)
    want_ids, want_sc = im.search(recs, 5, eta, pref)
    assert [int(r[0][1:]) for r in one] == want_ids[0].tolist()
    assert same_bits(np.array([r[1] for r in one], np.float32), want_sc[0])


@pytest.mark.parametrize("dim", [128, 768])
def test_rescored_search_against_the_float64_model(dim):
    """The decisive-gap rule of tests/parity.py on the model's own re-scored records: where the float64 blends of the k + 1 best
    candidates lie further apart than GAP the ids must be the model's, and every score lies within SCORE_TOL."""
    from parity import GAP, SCORE_TOL
    x, cols, q, idx = shadowed(dim)
    stored = idx._corpus.emb.cpu().numpy()
    decisive = total = 0
    for k, eta, pref in ((10, 0.0, 0.0), (10, 0.3, 0.2), (100, 0.3, 0.0)):
        rows, scores = idx.search_batch(q, k, eta, pref, approx=True)
        dflt, _ = idx.search_batch(q[:4], k, eta, pref)                  # None: the index has an int8 shadow (up to 4 queries)
        assert np.array_equal(rows[:4], dflt)
        recs, qn = model_records(idx, q, 2 * k)
        rec64 = im.rescore(recs, stored, qn)
        want_ids, want_sc = im.search(rec64, k, eta, pref)
        for j in range(q.shape[0]):
            s64 = stored[rec64["id"][j]].astype(np.float64) @ qn[j].astype(np.float64)
            adj = np.float64(np.float32(1 - eta)) * s64 + np.float64(np.float32(eta)) * rec64["dewi"][j]
            if pref:
                adj = adj + np.float64(np.float32(pref)) * rec64["ent"][j]
            top = np.sort(adj)[::-1][: k + 1]
            total += 1
            assert np.allclose(np.sort(scores[j]), np.sort(want_sc[j]), atol=SCORE_TOL, rtol=0)
            if np.min(top[:-1] - top[1:]) > GAP:
                decisive += 1
                assert rows[j].tolist() == want_ids[j].tolist(), (k, eta, pref, j)
            else:
                assert set(rows[j].tolist()) <= set(rec64["id"][j].tolist())
    assert decisive >= 0.5 * total, (decisive, total)


def test_exact_path_of_a_shadowed_index_is_unchanged():
    x, cols, q, idx = shadowed(128)
    plain = build_index(x, cols)
    for k in (10, 100):
        a = idx.search_batch(q, k, 0.3, 0.2, approx=False)
        b = plain.search_batch(q, k, 0.3, 0.2)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
        auto = idx.search_batch(q, k, 0.3, 0.2)                              # None, more than four queries: the exact path
        assert q.shape[0] > idx.APPROX_AUTO_MAX_BATCH and np.array_equal(auto[0], b[0]) and same_bits(auto[1], b[1])
    with pytest.raises(ValueError, match="int8_shadow=True"):
        plain.search_batch(q, 10, approx=True)
    with pytest.raises(ValueError, match="does not take a filter"):
        idx.search_batch(q, 10, approx=True, filter=np.ones(x.shape[0], bool))
    with pytest.raises(ValueError, match="at most 1024"):
        idx.search_batch(q, 600, approx=True)
    with pytest.raises(ValueError, match="exceeds the cut"):
        idx.search_batch(q, 30, candidates=20, approx=True)
    filtered = idx.search_batch(q, 5, 0.3, 0.0, filter=np.arange(x.shape[0]) % 2 == 0)       # None + filter: the exact path
    assert (filtered[0] % 2 == 0).all()


@pytest.mark.parametrize("k", [10, 100])
def test_embedding_like_corpus_rescored_answer_is_the_exact_one(k):
    from corpora import embedding_like
    if "emb" not in _cache:
        X, Q, _, _ = embedding_like(20000, 256, 3)
        _cache["emb"] = (Q, build_index(X, columns(X.shape[0], 1), cls="dewi", int8_shadow=True))
    Q, idx = _cache["emb"]
    assert Q.shape[0] == 32
    approx = idx.search_batch(Q, k, 0.0, 0.0, approx=True)
    exact = idx.search_batch(Q, k, 0.0, 0.0, approx=False)
    for j in range(32):
        a, e = {r[0] for r in approx[j]}, {r[0] for r in exact[j]}
        if a != e:                                            # a tie at the k-th place: compare by score
            sa, se = sorted(r[1] for r in approx[j]), sorted(r[1] for r in exact[j])
            assert np.allclose(sa, se, atol=1e-6, rtol=0), (j, sorted(a ^ e))
        assert len(approx[j]) == k


def test_save_load_round_trip(tmp_path):
    from dewi.backends import ExactIndex
    x, cols, q, idx = shadowed(128)
    idx.save(tmp_path / "ix")
    back = ExactIndex.load(tmp_path / "ix", int8_shadow=True)
    for rescore in (False, True):
        a = idx.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=rescore)
        b = back.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=rescore)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    assert np.array_equal(back._corpus.i8_codes.cpu().numpy(), idx._corpus.i8_codes.cpu().numpy())


def test_mutated_index_equals_a_fresh_build():
    n, dim = 1500, 128
    x = np.random.RandomState(5).randn(n + 40, dim).astype(np.float32)
    cols = columns(n + 40, 5)
    ids = [f"d{i:06d}" for i in range(n + 40)]
    idx = build_index(x[:n], {k: v[:n] for k, v in cols.items()}, int8_shadow=True)
    q = np.random.RandomState(6).randn(5, dim).astype(np.float32)
    idx.search_batch(q, 10, approx=True)                                  # the shadow is in use before the mutation
    idx.remove([ids[i] for i in range(0, 300, 7)])
    assert idx._corpus._i8_stale
    up = list(range(n, n + 40)) + [500, 501, 502]
    new_rows = x[up].copy()
    new_rows[-3:] = np.random.RandomState(7).randn(3, dim).astype(np.float32)
    idx.upsert_batch_columns([ids[i] for i in up], new_rows, {k: v[up] for k, v in cols.items()})
    assert idx._corpus._i8_stale
    # a fresh index of the same documents in the mutated index's row order
    raw = {ids[i]: x[i] for i in range(n + 40)}
    raw.update({ids[i]: r for i, r in zip(up, new_rows)})
    order = list(idx._doc_ids)
    pos = {d: i for i, d in enumerate(ids)}
    from dewi.backends import ExactIndex
    fresh = ExactIndex(dim, int8_shadow=True)
    fresh.add_batch_columns(order, np.stack([raw[d] for d in order]), {k: v[[pos[d] for d in order]] for k, v in cols.items()})
    fresh.build()
    for rescore in (False, True):
        a = idx.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=rescore)
        b = fresh.search_batch(q, 10, 0.3, 0.2, approx=True, rescore=rescore)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    assert not idx._corpus._i8_stale
    assert np.array_equal(idx._corpus.i8_codes.cpu().numpy(), fresh._corpus.i8_codes.cpu().numpy())
    assert same_bits(idx._corpus.i8_scales.cpu().numpy(), fresh._corpus.i8_scales.cpu().numpy())


def exact_dot_rows(n, dim, seed):
    """16 nonzeros of +-0.25 per row, 12 of them in the first 20 columns: unit rows whose inner products are exact in any
    order (tests/test_hip_diverse.py), with copies."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, dim), np.float32)
    for i in range(n):
        cols_ = np.concatenate([rs.choice(20, 12, replace=False), 20 + rs.choice(dim - 20, 4, replace=False)])
        rows[i, cols_] = rs.choice(np.array([0.25, -0.25], np.float32), 16)
    rows[1::8] = rows[0::8][: rows[1::8].shape[0]]
    return rows


@pytest.mark.parametrize("lam,max_sim", [(0.5, None), (1.0, 0.9), (0.3, 0.6)])
def test_diverse_search_over_the_int8_pool_equals_the_model(lam, max_sim):
    import torch
    from dewi._engine import records_to_numpy
    n, dim, k, c = 600, 64, 8, 40
    if "div" not in _cache:
        x = exact_dot_rows(n, dim, 3)
        _cache["div"] = (x, build_index(x, columns(n, 3), int8_shadow=True))
    x, idx = _cache["div"]
    q = x[[0, 17, 33]] + np.float32(0.125) * exact_dot_rows(3, dim, 4)
    rows, scores = idx.search_diverse_approx_batch(q, k, 0.3, 0.2, lam, c, max_sim)
    corpus = idx._corpus
    Q_dev = torch.from_numpy(q).cuda()
    recs = corpus.rescore_candidates_device(Q_dev, corpus.candidates_i8_device(Q_dev, c))
    torch.cuda.synchronize()
    recs = records_to_numpy(recs)
    stored = corpus.emb.cpu().numpy()
    want_ids, want_sc, _, kk = dm.diverse_rerank(recs, stored, k, 0.3, 0.2, lam, np.inf if max_sim is None else max_sim)
    assert np.array_equal(rows, want_ids)
    for j in range(3):
        assert same_bits(scores[j, :kk[j]], want_sc[j, :kk[j]]) and np.isnan(scores[j, kk[j]:]).all()
    res = idx.search_diverse_approx(q[0], k, 0.3, 0.2, lam, c, max_sim)
    assert [int(r[0][1:]) for r in res] == want_ids[0, :kk[0]].tolist()


def test_standalone_int8_corpus_equals_the_shadow_route():
    import torch
    x, cols, q, idx = shadowed(128)
    corpus = idx._corpus
    alone = corpus.to_int8()
    assert alone.corpus_bytes() == x.shape[0] * (128 + 4) and alone.n_rows == x.shape[0] and alone.dim == 128
    for k, cand in ((10, None), (5, 300)):
        a = alone.search_approx(q, k, 0.3, 0.2, cand)
        b = corpus.search_approx(q, k, 0.3, 0.2, cand, rescore=False)
        assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    with pytest.raises(NotImplementedError):
        alone.search_approx(q, 10, 0.3, 0.2, rescore=True)
    with pytest.raises(NotImplementedError):
        alone.search(q, 10)
    # a corpus without a shadow makes the codes for the copy only
    z = np.zeros(50)
    plain = type(corpus).from_host(unit_rows(50, 32, 1), z, z, z)
    copy = plain.to_int8()
    assert not plain.has_int8_shadow and copy.n_rows == 50
    with pytest.raises(ValueError, match="no int8 shadow"):
        plain.search_approx(np.zeros((1, 32), np.float32), 5)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ workspace contract
@pytest.mark.parametrize("dim,c,b", [(768, 20, 1), (768, 100, 5), (768, 300, 4), (128, 20, 5), (128, 300, 1)])
def test_workspace_contract(dim, c, b):
    """Results do not depend on what the workspace held; nothing outside the workspace, the records or (re-scoring) the
    record buffer is written."""
    import torch
    from dewi._engine import DeviceCorpus
    n = 2100
    z = np.zeros(n)
    corpus = DeviceCorpus.from_host(unit_rows(n, dim, dim + c), np.random.RandomState(1).rand(n), z, z).enable_int8_shadow()
    Q_dev = torch.from_numpy(np.random.RandomState(b).randn(b, dim).astype(np.float32)).cuda()
    corpus.candidates_i8_device(Q_dev, c)                       # the cache now holds this shape's workspace
    assert wsguard.guard(corpus) >= 1
    base = None
    for pattern in wsguard.PATTERNS:
        wsguard.poison(corpus, pattern, seed=c)
        out = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="records")
        corpus.candidates_i8_device(Q_dev, c, out=out.mid)
        torch.cuda.synchronize()
        out.check()
        wsguard.check(corpus)
        rescored = wsguard.GuardedOutput((b, c, 4), torch.int32, "cuda", label="re-scored records")
        rescored.mid.copy_(out.mid)
        corpus.rescore_candidates_device(Q_dev, rescored.mid)
        torch.cuda.synchronize()
        rescored.check()
        wsguard.check(corpus, interior=False)
        got = (out.mid.clone(), rescored.mid.clone())
        if base is None:
            base = got
        wsguard.assert_bit_equal(got, base, f"pattern {pattern}")
    wsguard.release(corpus)

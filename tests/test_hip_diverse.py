"""GPU: diverse search — ``dewi_diverse_rerank`` (csrc/diverse.hip) and the layers above it.

1. Bit for bit against tests/diverse_model.py at the ABI level, on records built on the host and corpus rows whose inner
   products are exact in ANY summation order (16 nonzeros of +-0.25: norm exactly 1, dots multiples of 1/16; exact in bf16
   too), so that the model's float64 Gram matrix, rounded, is the device's fp32 g whatever order it sums in.  Ids, scores and
   ``d_out_mmr`` are compared as bits (NaN == NaN), the prefill from ``kk`` on included.
2. The lambda = 1 invariant on gaussian corpora: ``search_diverse_device(mmr_lambda=1)`` == ``merge_rerank_device`` of the same
   ``candidates_device`` records == (one fp32 query) ``search(candidates=c)``.
3. End to end against the float64 model on the device's own records, for the queries the float64 model decides by a margin.
4. Behaviour through ``ExactIndex`` / ``DewiIndex`` / ``IVFIndex`` on a corpus with planted clusters of copies.
"""
import itertools

import numpy as np
import pytest

import diverse_model as dm
import rerank_model as rm

pytestmark = pytest.mark.gpu

INF = float("inf")
N_SYN = 512
NAN_ROW = 7
CS = [1, 7, 64, 65, 200, 1024]
BS = [1, 5, 37]
LAMS = [0.0, 0.3, 0.5, 1.0]
MAX_SIMS = [INF, 0.9, 0.25]
# (name, bf16, dim, rows): the wide one is beyond the columns the kernel stages in LDS (it reads both rows from memory)
CORPORA = [("f32_64", False, 64, N_SYN), ("f32_50", False, 50, N_SYN), ("f32_768", False, 768, N_SYN), ("bf16_64", True, 64, N_SYN),
           ("bf16_100", True, 100, N_SYN), ("f32_8200", False, 8200, 96)]
_cache = {}


def synthetic_rows(n, dim, seed):
    """[n, dim] fp32: 16 nonzeros of +-0.25 per row — 12 in the first 20 columns (so that rows overlap: dots from -0.75 to
    0.75 in steps of 1/16), 4 in the rest, the LAST column among them for every other row (the tail of a row that is not whole
    16-byte units) —, every 8th row an exact copy of its predecessor, one all-NaN row."""
    rs = np.random.RandomState(seed)
    rows = np.zeros((n, dim), np.float32)
    for i in range(n):
        head = rs.choice(20, 12, replace=False)
        tail = 20 + rs.choice(dim - 20, 4, replace=False)
        if i % 2:
            tail[0] = dim - 1
            while len(set(tail.tolist())) < 4:
                tail[1:] = 20 + rs.choice(dim - 21, 3, replace=False)
        rows[i, np.concatenate([head, tail])] = rs.choice(np.array([0.25, -0.25], np.float32), 16)
    rows[1::8] = rows[0::8][: rows[1::8].shape[0]]
    rows[NAN_ROW] = np.nan
    return rows


def corpus(name):
    """(host rows fp32 [n, dim], device tensor [n, dim] that starts at an odd row of a larger buffer, fp32 Gram matrix)"""
    import torch
    if name not in _cache:
        _, bf16, dim, n = next(c for c in CORPORA if c[0] == name)
        rows = synthetic_rows(n, dim, seed=dim)
        assert np.allclose(np.nansum(rows.astype(np.float64) ** 2, axis=1)[np.arange(n) != NAN_ROW], 1.0, atol=0)
        big = torch.zeros((n + 3, dim), dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        big[3:] = torch.from_numpy(rows).cuda()          # (+-0.25, 0 and NaN are exact in bf16)
        with np.errstate(invalid="ignore"):
            gram = (rows.astype(np.float64) @ rows.astype(np.float64).T).astype(np.float32)
        _cache[name] = (rows, big[3:], gram)
    return _cache[name]


def make_records(rs, b, c, k, n_rows, id_offset):
    """[b][c] records in no particular order (rank = position): values with ties, +-0, +-inf and NaN; padding tails (query 0:
    fewer valid records than k where k > 1); some ids outside the rows of the shard."""
    sims = np.array([0.75, 0.5, 0.5, 0.25, 0.0, -0.0, -0.5, 0.625, 0.375], np.float32)
    recs = np.zeros((b, c), rm.RECORD)
    for q in range(b):
        recs["sim"][q] = rs.choice(sims, c)
        recs["dewi"][q] = rs.choice(np.array([0.125, 0.25, 0.5, 0.875, -0.0], np.float32), c)
        recs["ent"][q] = rs.rand(c).astype(np.float32)
        for col, p in (("sim", 0.03), ("dewi", 0.03), ("ent", 0.02)):
            for v in (np.nan, np.inf, -np.inf):
                recs[col][q][rs.rand(c) < p] = v
        recs["id"][q] = (rs.permutation(n_rows)[:c] if c <= n_rows else rs.randint(0, n_rows, c)) + id_offset
        bad = rs.rand(c) < 0.06
        recs["id"][q][bad] = rs.choice(np.array([id_offset - 1, id_offset + n_rows, id_offset + n_rows + 5, 2 ** 31 - 1, 3]), int(bad.sum()))
        n_valid = c
        if q == 0 and k > 1:
            n_valid = k // 2
        elif q % 3 == 1:
            n_valid = rs.randint(1, c + 1)
        recs[q, n_valid:] = (-np.inf, 0.0, 0.0, -1)
    return recs


def run_abi(emb, recs, k, eta, pref, lam, max_sim, id_offset, want_mmr=True):
    """``dewi_diverse_rerank`` on prefilled outputs (ids -7, scores 123, mmr 321)."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    b, c = recs.shape
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(b, c, 4)).cuda()
    ids = torch.full((b, k), -7, dtype=torch.int64, device="cuda")
    sc = torch.full((b, k), 123.0, dtype=torch.float32, device="cuda")
    mmr = torch.full((b, k), 321.0, dtype=torch.float32, device="cuda")
    assert lib.dewi_diverse_workspace_bytes(b, c, int(emb.shape[1])) == 0
    nat.check(lib.dewi_diverse_rerank(emb.data_ptr(), 1 if emb.dtype == torch.bfloat16 else 0, int(emb.shape[0]), int(emb.shape[1]),
                                      nat.ptr(d_recs), b, c, k, float(eta), float(pref), float(lam), float(max_sim), int(id_offset),
                                      nat.ptr(ids), nat.ptr(sc), nat.ptr(mmr) if want_mmr else None, None, 0, nat.stream_ptr()))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), mmr.cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])


def model_outputs(recs, rows, gram, k, eta, pref, lam, max_sim, id_offset):
    ids, sc, mmr, kk = dm.diverse_rerank(recs, rows, k, eta, pref, lam, max_sim, id_offset, gram=gram)
    for q in range(recs.shape[0]):
        ids[q, kk[q]:], sc[q, kk[q]:], mmr[q, kk[q]:] = -7, 123.0, 321.0
    return ids, sc, mmr, kk


def compare(got, want, what):
    for q in range(want[0].shape[0]):
        assert got[0][q].tolist() == want[0][q].tolist(), f"{what} query {q}: ids {got[0][q].tolist()} want {want[0][q].tolist()}"
        assert bits_equal(got[1][q], want[1][q]), f"{what} query {q}: scores {got[1][q].tolist()} want {want[1][q].tolist()}"
        assert bits_equal(got[2][q], want[2][q]), f"{what} query {q}: mmr {got[2][q].tolist()} want {want[2][q].tolist()}"


def plan(c):
    """(k, B, lambda, max_sim, id_offset, eta, pref) over every (lambda, max_sim), the k and B rotating; B * k is kept
    small (the model is a Python loop per step)."""
    ks = sorted({1, max(1, c // 2), c})
    out = []
    for i, (lam, ms) in enumerate(itertools.product(LAMS, MAX_SIMS)):
        li, mi = divmod(i, len(MAX_SIMS))
        k = ks[(mi + li) % len(ks)]
        b = BS[(mi + 2 * li) % 3]
        while b * k > 8000 and b > 1:
            b = BS[BS.index(b) - 1]
        out.append((k, b, lam, ms, [0, 1000][i % 2], [0.3, 0.0, 1.0][i % 3], [0.0, 0.25][(i // 2) % 2]))
    return out


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("name", [x[0] for x in CORPORA])
def test_rerank_equals_the_model_bit_for_bit(name, c):
    rows, emb, gram = corpus(name)
    if c == 1024 and rows.shape[1] > 1000:
        plans = plan(c)[:4]            # (the wide rows: fewer of the longest runs)
    else:
        plans = plan(c)
    seen_short = seen_cut = False
    for i, (k, b, lam, ms, id_offset, eta, pref) in enumerate(plans):
        rs = np.random.RandomState(1000 * CS.index(c) + i)
        recs = make_records(rs, b, c, k, rows.shape[0], id_offset)
        want = model_outputs(recs, rows, gram, k, eta, pref, lam, ms, id_offset)
        got = run_abi(emb, recs, k, eta, pref, lam, ms, id_offset)
        compare(got, want, f"{name} c {c} k {k} B {b} lambda {lam} max_sim {ms} offset {id_offset}")
        seen_short |= bool((want[3] < k).any())
        seen_cut |= ms != INF and bool((want[3] < np.minimum(k, [len(dm.valid_records(r, rows.shape[0], id_offset)) for r in recs])).any())
    if c >= 7:
        assert seen_short, "no query was left with a prefilled tail"
    if c >= 64:
        assert seen_cut, "max_sim never shortened a result"


def test_out_of_range_ids_are_skipped_and_mmr_is_optional():
    rows, emb, gram = corpus("f32_64")
    recs = np.zeros((1, 6), rm.RECORD)
    recs[0] = [(0.9, 0.5, 0.1, 1010), (0.8, 0.5, 0.1, 999), (0.7, 0.5, 0.1, 1000 + N_SYN), (0.6, 0.5, 0.1, 5), (0.5, 0.5, 0.1, 1020),
               (-np.inf, 0.0, 0.0, -1)]
    got = run_abi(emb, recs, 4, 0.3, 0.0, 0.5, INF, 1000, want_mmr=False)
    assert sorted(got[0][0, :2].tolist()) == [1010, 1020] and got[0][0, 2:].tolist() == [-7, -7]
    assert (got[1][0, 2:] == 123.0).all() and (got[2] == 321.0).all()          # mmr NULL: never written
    compare(got[:2] + (np.full((1, 4), 321.0, np.float32),),
            model_outputs(recs, rows, gram, 4, 0.3, 0.0, 0.5, INF, 1000)[:2] + (np.full((1, 4), 321.0, np.float32),), "out of range")


def test_element_aligned_base_of_whole_unit_rows():
    """Rows of whole 16-byte units at a base address that is only element-aligned: the element-load path, the same bits."""
    import torch
    for name in ("f32_64", "bf16_64"):
        rows, emb, gram = corpus(name)
        flat = torch.zeros(emb.numel() + 1, dtype=emb.dtype, device="cuda")
        view = flat[1:].view(emb.shape)
        view.copy_(emb)
        assert view.data_ptr() % 16 != 0
        recs = make_records(np.random.RandomState(5), 5, 65, 32, rows.shape[0], 0)
        want = model_outputs(recs, rows, gram, 32, 0.3, 0.25, 0.5, 0.9, 0)
        compare(run_abi(view, recs, 32, 0.3, 0.25, 0.5, 0.9, 0), want, name + " element-aligned")
        compare(run_abi(emb, recs, 32, 0.3, 0.25, 0.5, 0.9, 0), want, name + " aligned")


@pytest.mark.parametrize("name", ["f32_50", "bf16_64"])
def test_a_query_does_not_depend_on_its_place_in_the_batch(name):
    rows, emb, gram = corpus(name)
    recs = make_records(np.random.RandomState(9), 37, 200, 100, rows.shape[0], 0)
    recs[30] = recs[2]
    got = run_abi(emb, recs, 100, 0.3, 0.0, 0.3, 0.9, 0)
    alone = run_abi(emb, recs[2:3], 100, 0.3, 0.0, 0.3, 0.9, 0)
    assert got[0][2].tolist() == got[0][30].tolist() == alone[0][0].tolist()
    for x, y in zip(got[1:], alone[1:]):
        assert bits_equal(x[2], y[0]) and bits_equal(x[30], y[0])


# ------------------------------------------------------------------------------------------------ gaussian corpora
def gaussian_corpus(n, dim, seed, bf16=False, copies=False):
    """DeviceCorpus of gaussian unit rows (``copies``: every 16th row gets a near-copy, noise 0.02, in the next row)."""
    from dewi import _engine as eng
    key = ("gauss", n, dim, seed, bf16, copies)
    if key not in _cache:
        rs = np.random.RandomState(seed)
        x = rs.randn(n, dim).astype(np.float32)
        if copies:
            x[1::16] = x[0::16] + 0.02 * np.linalg.norm(x[0::16], axis=1, keepdims=True) / np.sqrt(dim) * rs.randn(*x[0::16].shape).astype(np.float32)
        dewi = rs.rand(n)
        cp = eng.DeviceCorpus.from_host(x, dewi, rs.rand(n), rs.rand(n))
        _cache[key] = (cp.to_bf16() if bf16 else cp, x)
    return _cache[key]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_lambda_one_is_the_plain_search_over_the_pool(bf16):
    import torch
    from dewi import _engine as eng
    cp, x = gaussian_corpus(4096, 64, 3, bf16=bf16)
    rs = np.random.RandomState(4)
    for b, k, c, eta, pref in [(5, 10, 40, 0.3, 0.0), (1, 10, 40, 0.3, 0.2), (37, 20, 65, 0.5, 0.0), (1, 40, 40, 0.0, 0.0)]:
        q = torch.from_numpy((x[rs.randint(0, 4096, b)] + 0.1 * rs.randn(b, 64)).astype(np.float32)).cuda()
        recs = cp.candidates_device(q, c).clone()
        want_ids, want_sc = eng.merge_rerank_device(recs.unsqueeze(0), c, k, eta, pref)
        ids, sc = cp.search_diverse_device(q, k, eta, pref, mmr_lambda=1.0, candidates=c)
        torch.cuda.synchronize()
        assert torch.equal(ids, want_ids)
        assert bits_equal(sc.cpu().numpy(), want_sc.cpu().numpy())
        if b == 1 and not bf16:
            h_ids, h_sc = cp.search(q.cpu().numpy(), k, eta, pref, candidates=c)
            assert np.array_equal(h_ids, ids.cpu().numpy()) and bits_equal(h_sc, sc.cpu().numpy())
            d_ids, d_sc = cp.search_diverse(q.cpu().numpy(), k, eta, pref, mmr_lambda=1.0, candidates=c)
            assert np.array_equal(d_ids, h_ids) and bits_equal(d_sc, h_sc)


def test_device_entry_point_checks_its_arguments():
    import torch
    from dewi import _engine as eng
    cp, x = gaussian_corpus(4096, 64, 3)
    q = torch.from_numpy(x[:2].copy()).cuda()
    with pytest.raises(NotImplementedError):
        cp.search_diverse_device(q, 10, 0.3, 0.0, candidates=1025)
    with pytest.raises(ValueError):
        cp.search_diverse_device(q, 50, 0.3, 0.0, candidates=40)
    with pytest.raises(ValueError):
        cp.search_diverse_device(q, 10, 0.3, 0.0, mmr_lambda=1.5)
    with pytest.raises(ValueError):
        cp.search_diverse_device(q[:, :32].contiguous(), 10, 0.3, 0.0)
    assert tuple(cp.search_diverse_device(q, 0, 0.3, 0.0)[0].shape) == (2, 0)
    ids, _ = cp.search_diverse_device(q, 300, 0.3, 0.0)                  # default pool 4k = 1200, capped at 1024
    assert tuple(ids.shape) == (2, 300) and int((ids >= 0).sum()) == 600
    l2 = eng.DeviceCorpus(cp.emb, cp.dewi32, cp.ent32, space="l2")
    with pytest.raises(NotImplementedError):
        l2.search_diverse_device(q, 10, 0.3, 0.0)


E2E = [(4096, 64), (4096, 50), (2048, 768)]
MARGIN = 2e-6


@pytest.mark.parametrize("lam,max_sim", [(0.3, None), (0.5, None), (0.7, None), (0.5, 0.9)])
@pytest.mark.parametrize("shape", E2E, ids=lambda s: "x".join(map(str, s)))
def test_end_to_end_against_the_float64_model(shape, lam, max_sim):
    """The device's own candidate records, the stored rows' float64 Gram matrix, the selection in float64.  A query is
    DECISIVE when at every step the float64 margin between the best and the second eligible m exceeds 2e-6 (the fp32 error of
    m: a few ulp of values below 1, ~2e-7, on each side) and every pen is further than that from max_sim; a decisive query's
    picks must equal the model's in order.  At least 80 % of the queries must be decisive (on the CPU the float32 and float64
    models alone agreed on all such queries, 63-64 of 64 being decisive)."""
    import torch
    n, dim = shape
    k, c, eta, pref, b = 10, 40, 0.3, 0.0, 32
    cp, x = gaussian_corpus(n, dim, 21, copies=True)
    rs = np.random.RandomState(8)
    src = np.concatenate([16 * rs.randint(0, n // 16, b // 2), rs.randint(0, n, b - b // 2)])    # half of them rows with a copy
    q = (x[src] + 0.3 * np.linalg.norm(x[src], axis=1, keepdims=True) / np.sqrt(dim) * rs.randn(b, dim)).astype(np.float32)
    q_dev = torch.from_numpy(q).cuda()
    recs = eng_records(cp, q_dev, c)
    ids, sc = cp.search_diverse_device(q_dev, k, eta, pref, mmr_lambda=lam, candidates=c, max_sim=max_sim)
    torch.cuda.synchronize()
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    stored = cp.emb.cpu().numpy().astype(np.float64)
    decisive = 0
    for j in range(b):
        valid = recs[j][recs[j]["id"] >= 0]
        assert valid.shape[0] == c
        adj = rm.blend(valid["sim"], valid["dewi"], valid["ent"], eta, pref)
        adj_of = dict(zip(valid["id"].tolist(), adj.tolist()))
        margins = []
        m_ids, m_sc, _ = dm.diverse_one(recs[j], stored, k, eta, pref, lam, INF if max_sim is None else max_sim,
                                        gram=lambda local: stored[local] @ stored[local].T, exact=True, margins=margins)
        kk = int((ids[j] >= 0).sum())
        got = ids[j, :kk].tolist()
        assert (ids[j, kk:] == -1).all() and np.isnan(sc[j, kk:]).all()
        if all(g > MARGIN and p > MARGIN for g, p in margins):
            decisive += 1
            assert got == m_ids.tolist(), f"query {j}: {got} want {m_ids.tolist()}"
            assert np.max(np.abs(sc[j, :kk] - m_sc)) <= 1e-5
        assert len(set(got)) == kk and set(got) <= set(adj_of)
        assert sc[j, :kk].tolist() == [np.float32(adj_of[i]) for i in got]
    print(f"{shape} lambda {lam} max_sim {max_sim}: {decisive} of {b} queries decisive")
    assert decisive >= 0.8 * b


def eng_records(cp, q_dev, c):
    import torch
    from dewi import _engine as eng
    recs = cp.candidates_device(q_dev, c)
    torch.cuda.synchronize()
    return eng.records_to_numpy(recs)


# ------------------------------------------------------------------------------------------------ behaviour
CLUSTERS, COPIES, SINGLES, DIM = 40, 5, 400, 64


def clustered(cls, **kwargs):
    """An index of ``CLUSTERS`` x ``COPIES`` near-copies (noise 1e-3: similarity > 0.999) and ``SINGLES`` single documents."""
    import dewi_oracle as orc
    key = ("clustered", cls.__name__)
    if key not in _cache:
        rs = np.random.RandomState(31)
        centres = rs.randn(CLUSTERS, DIM).astype(np.float32)
        x = np.concatenate([np.repeat(centres, COPIES, axis=0) + 1e-3 * rs.randn(CLUSTERS * COPIES, DIM).astype(np.float32),
                            rs.randn(SINGLES, DIM).astype(np.float32)])
        label = np.concatenate([np.repeat(np.arange(CLUSTERS), COPIES), CLUSTERS + np.arange(SINGLES)])
        perm = rs.permutation(x.shape[0])
        x, label = x[perm], label[perm]
        n = x.shape[0]
        idx = cls(dim=DIM, **kwargs)
        names = [f"doc_{i:04d}" for i in range(n)]
        idx.add_batch_columns(names, x, orc.synth_payload_columns(n, seed=2))
        idx.build()
        queries = (centres[:8] + 0.05 * rs.randn(8, DIM)).astype(np.float32)
        _cache[key] = (idx, x, dict(zip(names, label.tolist())), queries)
    return _cache[key]


def struck(results, label, k):
    """The plain ranking with every result dropped whose cluster an earlier result already stands for."""
    out, seen = [], set()
    for r in results:
        if label[r[0]] not in seen:
            seen.add(label[r[0]])
            out.append(r)
    return out[:k]


def same_cluster_pairs(results, label):
    labs = [label[r[0]] for r in results]
    return sum(1 for i in range(len(labs)) for j in range(i) if labs[i] == labs[j])


def test_one_result_per_cluster_on_exact_index():
    from dewi.backends import ExactIndex
    from dewi.types import Payload
    idx, x, label, queries = clustered(ExactIndex)
    for q in queries:
        res = idx.search_diverse(q, k=10, eta=0.3, mmr_lambda=1.0, max_sim=0.95)
        plain = idx.search(q, k=40, eta=0.3, candidates=40)
        assert same_cluster_pairs(res, label) == 0
        want = struck(plain, label, 10)
        assert [r[0] for r in res] == [r[0] for r in want] and [r[1] for r in res] == [r[1] for r in want]
        assert all(isinstance(r[0], str) and isinstance(r[1], float) and isinstance(r[2], Payload) for r in res)
        assert [r[2] for r in res] == [r[2] for r in want]
        top = idx.search(q, k=10, eta=0.3)
        half = idx.search_diverse(q, k=10, eta=0.3, mmr_lambda=0.5)
        assert len(half) == 10 and same_cluster_pairs(top, label) >= 10          # the 5 copies of the query's cluster
        assert same_cluster_pairs(half, label) < same_cluster_pairs(top, label)
    rows, scores = idx.search_diverse_batch(queries, k=10, eta=0.3, mmr_lambda=1.0, max_sim=0.95)
    for j, q in enumerate(queries):
        assert [f"doc_{r:04d}" for r in rows[j]] == [r[0] for r in idx.search_diverse(q, k=10, eta=0.3, mmr_lambda=1.0, max_sim=0.95)]
    short = idx.search_diverse(queries[0], k=30, eta=0.3, mmr_lambda=1.0, candidates=30, max_sim=-1.0)
    assert len(short) == 1 and short[0][0] == idx.search(queries[0], k=1, eta=0.3, candidates=30)[0][0]


def test_one_result_per_cluster_through_the_facade_and_the_ivf_index():
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    facade, _, label, queries = clustered(DewiIndex, use_ann=False, rerank_eta=0.3)
    ivf, _, label_ivf, _ = clustered(IVFIndex, nlist=16, nprobe=2)
    assert label == label_ivf
    for q in queries:
        res = facade.search_diverse(q, k=10, mmr_lambda=1.0, max_sim=0.95)
        want = struck(facade._backend.search(q, 40, 0.3, 0.0, candidates=40), label, 10)
        assert same_cluster_pairs(res, label) == 0 and [(r[0], r[1]) for r in res] == [(r[0], r[1]) for r in want]
        assert same_cluster_pairs(facade.search_diverse(q, k=10), label) < same_cluster_pairs(facade.search(q, k=10), label)
        res = ivf.search_diverse(q, k=10, eta=0.3, mmr_lambda=1.0, max_sim=0.95)
        rows, scores = ivf._corpus.search(q[None, :], 40, 0.3, 0.0, candidates=40)               # the exact form: every row
        want = struck(ivf.results_for(rows, scores)[0], label, 10)
        assert same_cluster_pairs(res, label) == 0 and [(r[0], r[1]) for r in res] == [(r[0], r[1]) for r in want]
    batch = facade.search_diverse_batch(queries, k=10, mmr_lambda=1.0, max_sim=0.95)
    assert [[r[0] for r in row] for row in batch] == [[r[0] for r in facade.search_diverse(q, k=10, mmr_lambda=1.0, max_sim=0.95)]
                                                      for q in queries]

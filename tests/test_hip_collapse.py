"""GPU: collapsed search — ``dewi_collapse_rerank`` (csrc/collapse.hip), ``dewi_knn_candidates_filtered`` and the layers above.

1. The ABI bit for bit against tests/collapse_model.py on records built on the host: ids, scores, hits, counts and the
   unwritten tail (the prefill) compared as bits, NaN == NaN.  ``d_labels`` is the LAST ``n_rows`` elements of its buffer and the
   elements in front of it hold a label every query uses, so an out-of-range id that were looked up would change a result.
2. The identities on the device: nothing folded == ``merge_rerank_device``; one group, one result; the same bytes twice.
3. ``dewi_knn_candidates_filtered`` against ``dewi_knn_candidates`` / ``dewi_knn_rerank_filtered``.
4. Through ``ExactIndex`` / ``DewiIndex`` / ``IVFIndex`` on a corpus with planted clusters of exact copies.
"""
import numpy as np
import pytest

import collapse_model as cm
import rerank_model as rm
import wsguard

pytestmark = pytest.mark.gpu

N_ABI = 2560                       # rows of the ABI tests: more than the largest pool, 10240 bytes of labels
POISON_LABEL = 3                   # what the buffer holds in front of the labels: a group of every pattern below
CS = [1, 7, 64, 65, 200, 1024, 1025, 2048]
BS = [1, 5, 37]
ETAS = [(0.0, 0.0), (0.3, 0.0), (0.3, 0.2)]
PATTERNS = ["distinct", "equal", "negative", "few_large", "extremes", "nan_group"]
NAN_ROWS = 48                      # "nan_group": rows below this carry one label and every record of them a NaN similarity
_cache = {}


def make_records(rs, b, c, k, n_rows, id_offset, nan_rows=0, bad_ids=True, sort=False):
    """[b][c] records (rank = position): values with ties, +-0, +-inf and NaN in sim / dewi / ent; padding tails (query 0: fewer
    valid records than k where k > 1); ids outside the rows, id_offset - 1, id_offset + n_rows and 2^31 - 1 among them."""
    sims = np.array([0.75, 0.5, 0.5, 0.25, 0.0, -0.0, -0.5, 0.625, 0.375], np.float32)
    recs = np.zeros((b, c), rm.RECORD)
    for q in range(b):
        recs["sim"][q] = rs.choice(sims, c)
        recs["dewi"][q] = rs.choice(np.array([0.125, 0.25, 0.5, 0.875, -0.0], np.float32), c)
        recs["ent"][q] = rs.rand(c).astype(np.float32)
        for col, p in (("sim", 0.03), ("dewi", 0.03), ("ent", 0.02)):
            for v in (np.nan, np.inf, -np.inf):
                recs[col][q][rs.rand(c) < p] = v
        recs["id"][q] = rs.permutation(n_rows)[:c] + id_offset
        if nan_rows:
            recs["sim"][q][recs["id"][q] - id_offset < nan_rows] = np.nan
        if bad_ids:
            bad = rs.rand(c) < 0.06
            recs["id"][q][bad] = rs.choice(np.array([id_offset - 1, id_offset + n_rows, id_offset + n_rows + 5, 2 ** 31 - 1, 3]), int(bad.sum()))
        n_valid = c
        if q == 0 and k > 1:
            n_valid = k // 2
        elif q % 3 == 1:
            n_valid = rs.randint(1, c + 1)
        if sort:
            head = recs[q, :n_valid]
            recs[q, :n_valid] = head[rm.record_order(head)]
        recs[q, n_valid:] = (-np.inf, 0.0, 0.0, -1)
    return recs


def make_labels(rs, kind, n_rows):
    if kind == "distinct":
        return rs.permutation(n_rows).astype(np.int32)
    if kind == "equal":
        return np.full(n_rows, POISON_LABEL, np.int32)
    if kind == "negative":
        return (-1 - rs.randint(0, 3, n_rows)).astype(np.int32)
    if kind == "few_large":
        return np.where(rs.rand(n_rows) < 0.6, rs.randint(0, 5, n_rows), 100 + np.arange(n_rows)).astype(np.int32)
    if kind == "extremes":
        return rs.choice(np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], np.int64), n_rows).astype(np.int32)
    lab = np.where(rs.rand(n_rows) < 0.5, rs.randint(0, 6, n_rows), 100 + np.arange(n_rows)).astype(np.int32)
    lab[:NAN_ROWS] = 77
    return lab


def device_labels(labels):
    """The labels as the LAST elements of their device buffer; the 64 in front hold ``POISON_LABEL``."""
    import torch
    buf = torch.full((64 + labels.shape[0],), POISON_LABEL, dtype=torch.int32, device="cuda")
    buf[64:] = torch.from_numpy(labels).cuda()
    return buf, buf[64:]


def run_abi(recs, d_labels, n_rows, k, per_group, eta, pref, id_offset, want_hits=True, want_counts=True):
    """``dewi_collapse_rerank`` on prefilled outputs (ids -7, scores 123, hits -9, counts -5)."""
    import torch
    from dewi import _native as nat
    lib = nat.load_library()
    b, c = recs.shape
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(b, c, 4)).cuda()
    ids = torch.full((b, k), -7, dtype=torch.int64, device="cuda")
    sc = torch.full((b, k), 123.0, dtype=torch.float32, device="cuda")
    hits = torch.full((b, k), -9, dtype=torch.int32, device="cuda")
    counts = torch.full((b,), -5, dtype=torch.int32, device="cuda")
    assert lib.dewi_collapse_workspace_bytes(b, c) == 0
    nat.check(lib.dewi_collapse_rerank(nat.ptr(d_recs), b, c, nat.ptr(d_labels), int(n_rows), int(id_offset), int(k), int(per_group),
                                       float(eta), float(pref), nat.ptr(ids), nat.ptr(sc), nat.ptr(hits) if want_hits else None,
                                       nat.ptr(counts) if want_counts else None, None, 0, nat.stream_ptr()))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy(), hits.cpu().numpy(), counts.cpu().numpy()


def model_outputs(recs, labels, n_rows, k, per_group, eta, pref, id_offset):
    b = recs.shape[0]
    return cm.collapse_rerank(recs, labels, n_rows, k, per_group, eta, pref, id_offset, out_ids=np.full((b, k), -7, np.int64),
                              out_scores=np.full((b, k), 123.0, np.float32), out_hits=np.full((b, k), -9, np.int32),
                              out_counts=np.full(b, -5, np.int32))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint32)[~nan_a], b.view(np.uint32)[~nan_b])


def compare(got, want, what):
    for q in range(want[0].shape[0]):
        assert got[0][q].tolist() == want[0][q].tolist(), f"{what} query {q}: ids {got[0][q].tolist()} want {want[0][q].tolist()}"
        assert bits_equal(got[1][q], want[1][q]), f"{what} query {q}: scores {got[1][q].tolist()} want {want[1][q].tolist()}"
        assert got[2][q].tolist() == want[2][q].tolist(), f"{what} query {q}: hits {got[2][q].tolist()} want {want[2][q].tolist()}"
    assert got[3].tolist() == want[3].tolist(), f"{what}: counts {got[3].tolist()} want {want[3].tolist()}"


def plan(c):
    """(k, B, per_group, eta, pref, id_offset): every per_group x (eta, pref), the k, B and offset rotating so that every
    value of each meets every pool size."""
    ks = [1, min(10, c), c]
    out = []
    for i, (m, (eta, pref)) in enumerate((m, e) for m in (1, 2, 3, c) for e in ETAS):
        mi, ei = divmod(i, len(ETAS))
        out.append((ks[(mi + ei) % 3], BS[(mi + 2 * ei) % 3], m, eta, pref, [0, 1000][i % 2]))
    return out


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("c", CS)
def test_collapse_equals_the_model_bit_for_bit(c, kind):
    seen_short = seen_folded = False
    for i, (k, b, per_group, eta, pref, id_offset) in enumerate(plan(c)):
        rs = np.random.RandomState(1000 * CS.index(c) + 50 * PATTERNS.index(kind) + i)
        labels = make_labels(rs, kind, N_ABI)
        recs = make_records(rs, b, c, k, N_ABI, id_offset, nan_rows=NAN_ROWS if kind == "nan_group" else 0)
        keep, d_labels = device_labels(labels)
        want = model_outputs(recs, labels, N_ABI, k, per_group, eta, pref, id_offset)
        got = run_abi(recs, d_labels, N_ABI, k, per_group, eta, pref, id_offset)
        compare(got, want, f"c {c} {kind} k {k} B {b} per_group {per_group} eta {eta} pref {pref} offset {id_offset}")
        seen_short |= bool((want[3] < k).any())
        n_sel = np.array([len(cm.valid_records(r, N_ABI, id_offset)) for r in recs])
        seen_folded |= bool((want[3] < np.minimum(k, n_sel)).any())
    if c >= 7:
        assert seen_short, "no query was left with a prefilled tail"
    if c >= 64 and kind in ("equal", "few_large", "extremes", "nan_group"):
        assert seen_folded, "no record was ever folded"


def test_optional_outputs_may_be_null_and_out_of_range_ids_read_no_label():
    labels = np.array([POISON_LABEL + 1] * 8, np.int32)
    keep, d_labels = device_labels(labels)
    recs = np.zeros((1, 7), rm.RECORD)
    # offset 1000, 8 rows: 999 would read the poison label in front of the labels, 1008 the element behind the buffer
    recs[0] = [(0.9, 0.5, 0.1, 999), (0.8, 0.5, 0.1, 1001), (0.7, 0.5, 0.1, 1008), (0.6, 0.5, 0.1, 2 ** 31 - 1), (0.5, 0.5, 0.1, 5),
               (0.4, 0.5, 0.1, 1007), (-np.inf, 0.0, 0.0, -1)]
    got = run_abi(recs, d_labels, 8, 4, 1, 0.3, 0.0, 1000, want_hits=False, want_counts=False)
    assert got[0][0].tolist() == [1001, -7, -7, -7] and (got[2] == -9).all() and (got[3] == -5).all()
    got = run_abi(recs, d_labels, 8, 4, 2, 0.3, 0.0, 1000)
    assert got[0][0].tolist() == [1001, 1007, -7, -7] and got[2][0].tolist() == [2, 2, -9, -9] and got[3].tolist() == [2]
    compare(got, model_outputs(recs, labels, 8, 4, 2, 0.3, 0.0, 1000), "out of range")


@pytest.mark.parametrize("c", [7, 200, 1024, 1025, 2048])
def test_identities_on_the_device(c):
    import torch
    from dewi import _engine as eng
    rs = np.random.RandomState(c)
    b, k = 5, min(10, c)
    recs = make_records(rs, b, c, k, N_ABI, 0, bad_ids=False, sort=True)
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.int32).reshape(b, c, 4)).cuda()
    m_ids = torch.full((b, k), -7, dtype=torch.int64, device="cuda")
    m_sc = torch.full((b, k), 123.0, dtype=torch.float32, device="cuda")
    eng.merge_rerank_device(d_recs.unsqueeze(0), c, k, 0.3, 0.2, m_ids, m_sc)
    torch.cuda.synchronize()
    for kind, per_group in (("few_large", c), ("distinct", 1), ("negative", 1)):
        keep, d_labels = device_labels(make_labels(rs, kind, N_ABI))
        got = run_abi(recs, d_labels, N_ABI, k, per_group, 0.3, 0.2, 0)
        assert got[0].tolist() == m_ids.cpu().numpy().tolist(), (kind, per_group)
        assert bits_equal(got[1], m_sc.cpu().numpy()), (kind, per_group)
    keep, d_labels = device_labels(make_labels(rs, "equal", N_ABI))
    one = run_abi(recs, d_labels, N_ABI, k, 1, 0.3, 0.2, 0)
    best, _ = eng.merge_rerank_device(d_recs.unsqueeze(0), c, 1, 0.3, 0.2)          # (k = 1: a NaN score is the best)
    assert one[3].tolist() == [1] * b and one[0][:, 0].tolist() == best.cpu().numpy()[:, 0].tolist()
    assert (one[0][:, 1:] == -7).all()
    n_sel = [len(cm.valid_records(r, N_ABI, 0)) for r in recs]
    assert one[2][:, 0].tolist() == n_sel
    again = run_abi(recs, d_labels, N_ABI, k, 1, 0.3, 0.2, 0)
    for x, y in zip(one, again):
        assert x.tobytes() == y.tobytes()


# ------------------------------------------------------------------------------------------------ filtered candidate records
def gaussian_corpus(n, dim, seed):
    from dewi import _engine as eng
    key = ("gauss", n, dim, seed)
    if key not in _cache:
        rs = np.random.RandomState(seed)
        x = rs.randn(n, dim).astype(np.float32)
        x[1::16] = x[0::16]                                         # exact copies: ties on the similarity
        _cache[key] = (eng.DeviceCorpus.from_host(x, rs.rand(n), rs.rand(n), rs.rand(n)), x)
    return _cache[key]


def list_mask(rs, n, kind):
    if kind == "full":
        return np.ones(n, bool)
    if kind == "half":
        return rs.rand(n) < 0.5
    m = np.zeros(n, bool)
    m[rs.choice(n, 3, replace=False)] = True
    return m


@pytest.mark.parametrize("kind", ["full", "half", "three"])
@pytest.mark.parametrize("b", [1, 4, 9])
@pytest.mark.parametrize("n,dim", [(512, 64), (512, 50), (512, 768), (4096, 64), (4096, 50), (4096, 768)])
def test_filtered_candidate_records(n, dim, b, kind):
    import torch
    from dewi import _engine as eng
    cp, x = gaussian_corpus(n, dim, dim + n)
    rs = np.random.RandomState(7 * b + n + len(kind))
    mask = list_mask(rs, n, kind)
    f = cp.make_filter(mask)
    n_a = int(mask.sum())
    q = torch.from_numpy((x[rs.randint(0, n, b)] + 0.1 * rs.randn(b, dim)).astype(np.float32)).cuda()
    c = 40
    c_local = min(c, n_a)
    recs_d = cp.candidates_filtered_device(q, c, f).clone()
    torch.cuda.synchronize()
    recs = eng.records_to_numpy(recs_d)
    # padding lies behind c_local; everything in front is a row of the list, in the records' order
    assert (recs["id"][:, c_local:] == -1).all() and np.isneginf(recs["sim"][:, c_local:]).all()
    assert (recs["dewi"][:, c_local:] == 0).all() and (recs["ent"][:, c_local:] == 0).all()
    assert mask[recs["id"][:, :c_local]].all()
    for j in range(b):
        assert rm.record_order(recs[j]).tolist() == list(range(c_local))
    if b == 1 and kind == "full":
        plain = cp.candidates_device(q, c).clone()
        torch.cuda.synchronize()
        assert torch.equal(plain, recs_d)
    if n <= 2048:
        for j in range(b):                                          # the one-query unfiltered records over every row
            every = eng.records_to_numpy(cp.candidates_device(q[j:j + 1], n).clone())[0]
            want = every[mask[every["id"]]][:c_local]
            assert want.tobytes() == recs[j, :c_local].tobytes(), f"query {j}"
    # steps 3-5 on the records are the filtered search with this cut
    k = min(10, c_local)
    m_ids, m_sc = eng.merge_rerank_device(recs_d.unsqueeze(0), c, k, 0.3, 0.2)
    s_ids, s_sc = cp.search_device(q, k, 0.3, 0.2, candidates=c, filter=f)
    torch.cuda.synchronize()
    assert torch.equal(m_ids, s_ids) and bits_equal(m_sc.cpu().numpy(), s_sc.cpu().numpy())
    # results do not depend on what the workspace held on entry
    if (n, dim) in ((512, 50), (4096, 768)):
        assert wsguard.guard(cp) >= 1
        try:
            for pattern in ("0xff", "random"):
                wsguard.poison(cp, pattern, seed=b)
                again = cp.candidates_filtered_device(q, c, f).clone()
                torch.cuda.synchronize()
                wsguard.check(cp, interior=False)
                wsguard.assert_bit_equal((again,), (recs_d,), f"workspace filled with {pattern}")
        finally:
            wsguard.release(cp)
            cp.drop_cached_workspaces()


def test_filtered_records_of_an_empty_list_and_a_nonzero_offset():
    import torch
    from dewi import _engine as eng
    cp, x = gaussian_corpus(512, 64, 576)
    q = torch.from_numpy(x[:2].copy()).cuda()
    empty = eng.records_to_numpy(cp.candidates_filtered_device(q, 5, cp.make_filter(np.zeros(512, bool))))
    assert (empty["id"] == -1).all() and np.isneginf(empty["sim"]).all()
    shard = eng.DeviceCorpus(cp.emb, cp.dewi32, cp.ent32, id_offset=7000)
    mask = np.arange(512) % 3 == 0
    a = eng.records_to_numpy(cp.candidates_filtered_device(q, 20, cp.make_filter(mask)))
    b = eng.records_to_numpy(shard.candidates_filtered_device(q, 20, shard.make_filter(mask)))
    assert (b["id"] == a["id"] + 7000).all() and a["sim"].tobytes() == b["sim"].tobytes()
    with pytest.raises(NotImplementedError, match="2049"):
        cp.candidates_filtered_device(q, 2049, cp.make_filter(mask))


# ------------------------------------------------------------------------------------------------ through the indexes
N_IDX, DIM, BIG = 2000, 64, 300


def planted(cls, **kwargs):
    """2 000 gaussian documents: one cluster of ``BIG`` exact copies, 30 clusters of 6, singles; a random "source" per
    document.  -> (index, rows, cluster label per row, sources, queries)."""
    import dewi_oracle as orc
    key = ("planted", cls.__name__, tuple(sorted(kwargs.items())))
    if key not in _cache:
        rs = np.random.RandomState(17)
        centres = rs.randn(31, DIM).astype(np.float32)
        n_single = N_IDX - BIG - 30 * 6
        x = np.concatenate([np.repeat(centres[:1], BIG, axis=0), np.repeat(centres[1:], 6, axis=0), rs.randn(n_single, DIM).astype(np.float32)])
        cluster = np.concatenate([np.zeros(BIG, np.int64), np.repeat(np.arange(1, 31), 6), 31 + np.arange(n_single)])
        perm = rs.permutation(N_IDX)
        x, cluster = x[perm], cluster[perm]
        sources = [f"site{v}.org" for v in rs.randint(0, 40, N_IDX)]
        idx = cls(dim=DIM, **kwargs)
        idx.add_batch_columns([f"doc_{i:04d}" for i in range(N_IDX)], x, orc.synth_payload_columns(N_IDX, seed=2))
        idx.build()
        queries = (centres[:6] + 0.05 * rs.randn(6, DIM)).astype(np.float32)
        _cache[key] = (idx, x, cluster, sources, queries)
    return _cache[key]


def model_rows(cp, q, labels, k, per_group, eta, pref, c, f=None, approx=False):
    import torch
    from dewi import _engine as eng
    q_dev = torch.from_numpy(q).cuda()
    if approx:
        recs = cp.rescore_candidates_device(q_dev, cp.candidates_i8_device(q_dev, c))
    else:
        recs = cp.candidates_device(q_dev, c) if f is None else cp.candidates_filtered_device(q_dev, c, f)
    torch.cuda.synchronize()
    return cm.collapse_rerank(eng.records_to_numpy(recs.clone()), labels, cp.n_rows, k, per_group, eta, pref, cp.id_offset)


def factorised(values):
    codes = {}
    return np.array([codes.setdefault(v, len(codes)) for v in values], np.int32)


def test_index_search_equals_the_model_on_the_device_records():
    from dewi.backends import ExactIndex
    idx, x, cluster, sources, queries = planted(ExactIndex)
    cp = idx._corpus
    dup = idx.duplicate_groups(0.999)
    assert dup.n_groups == len(set(cluster.tolist()))
    mask = np.random.RandomState(3).rand(N_IDX) < 0.5
    by_doc = {f"doc_{i:04d}": s for i, s in enumerate(sources) if i % 2 == 0}
    doc_labels = np.full(N_IDX, -1, np.int32)                       # documents the mapping does not name are ungrouped
    doc_labels[0::2] = factorised(sources[0::2])
    forms = [(dup, dup.labels.astype(np.int32)), (sources, factorised(sources)), (by_doc, doc_labels),
             (idx.make_groups(sources), factorised(sources))]
    for groups, labels in forms:
        for per_group, c, filt in ((1, 40, None), (2, 400, None), (1, 40, mask), (3, 1025, mask)):
            f = None if filt is None else idx.make_filter(filt)
            rows, scores, hits = idx.search_collapsed_batch(queries, 10, 0.3, 0.2, groups=groups, per_group=per_group, candidates=c,
                                                            filter=f, return_hits=True)
            want = model_rows(cp, queries, labels, 10, per_group, 0.3, 0.2, min(c, N_IDX if f is None else f.n_allowed), f)
            assert rows.tolist() == want[0].tolist() and bits_equal(scores, want[1]) and hits.tolist() == want[2].tolist()
            if f is not None:
                assert mask[rows[rows >= 0]].all()
    # the single form: tuples like search, padding dropped
    res, h = idx.search_collapsed(queries[0], 10, 0.3, 0.2, groups=dup, candidates=40, return_hits=True)
    rows, scores, hits = idx.search_collapsed_batch(queries[:1], 10, 0.3, 0.2, groups=dup, candidates=40, return_hits=True)
    n_real = int((rows[0] >= 0).sum())
    assert [r[0] for r in res] == [f"doc_{i:04d}" for i in rows[0, :n_real]] and h == hits[0, :n_real].tolist()
    assert [r[1] for r in res] == [float(s) for s in scores[0, :n_real]]
    assert idx.search_collapsed(queries[0], 10, 0.3, 0.2, groups=dup, candidates=40) == res


def test_one_document_per_cluster_and_hits_count_the_cluster():
    from dewi.backends import ExactIndex
    idx, x, cluster, sources, queries = planted(ExactIndex)
    dup = idx.duplicate_groups(0.999)
    rows, scores, hits = idx.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=dup, candidates=400, return_hits=True)
    for j in range(queries.shape[0]):
        got = rows[j][rows[j] >= 0]
        assert len(set(cluster[got].tolist())) == len(got) == 10
    # query 0 sits inside the cluster of 300 copies: all of them are the 300 best of a pool of 400
    assert cluster[rows[0, 0]] == 0 and hits[0, 0] == BIG
    plain = idx.search_batch(queries[1:2], 10, 0.3, 0.0, candidates=400)[0][0]
    assert cluster[rows[1, 0]] == 1 and hits[1, 0] == 6 and rows[1, 0] == plain[0]      # the group's best FOR THE QUERY leads
    two = idx.search_collapsed_batch(queries[1:2], 10, 0.3, 0.0, groups=dup, per_group=2, candidates=400)[0][0]
    assert (cluster[two] == 1).sum() == 2


def test_widen_grows_the_pool_until_k_results():
    from dewi.backends import ExactIndex
    idx, x, cluster, sources, queries = planted(ExactIndex)
    dup = idx.make_groups(cluster)
    queries = queries[:4]                                           # (batches the row kernels serve, whatever their size)
    rows, scores, pool = idx.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=dup, candidates=16, widen=True, return_pool=True)
    narrow = idx.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=dup, candidates=16)[0]
    assert (narrow[0] >= 0).sum() == 1 and (rows >= 0).all()
    assert pool[0] == 1024 and (pool[1:] <= 64).all() and (pool >= 16).all()
    for j in range(queries.shape[0]):                               # by definition: the answer of the final pool, not widened
        r, s = idx.search_collapsed_batch(queries[j:j + 1], 10, 0.3, 0.0, groups=dup, candidates=int(pool[j]))
        assert r[0].tolist() == rows[j].tolist() and bits_equal(s[0], scores[j])


def test_a_cluster_larger_than_the_cap_leaves_the_row_short():
    import dewi_oracle as orc
    from dewi.backends import ExactIndex
    rs = np.random.RandomState(5)
    n, copies = 2400, 2100
    x = rs.randn(n, 16).astype(np.float32)
    x[:copies] = x[0]
    idx = ExactIndex(dim=16)
    idx.add_batch_columns([f"d{i}" for i in range(n)], x, orc.synth_payload_columns(n, seed=3))
    labels = np.where(np.arange(n) < copies, 0, -1)
    rows, scores, hits, pool = idx.search_collapsed_batch(x[:1], 5, 0.3, 0.0, groups=labels, widen=True, return_hits=True, return_pool=True)
    assert pool.tolist() == [2048] and (rows[0] >= 0).sum() == 1 and rows[0, 1:].tolist() == [-1] * 4
    assert hits[0].tolist() == [2048, 0, 0, 0, 0] and np.isnan(scores[0, 1:]).all()


def test_prepared_groups_go_stale_and_bad_calls_raise():
    import dewi_oracle as orc
    from dewi.backends import ExactIndex
    rs = np.random.RandomState(6)
    n = 300
    x = rs.randn(n, 32).astype(np.float32)
    idx = ExactIndex(dim=32)
    idx.add_batch_columns([f"d{i}" for i in range(n)], x, orc.synth_payload_columns(n, seed=4))
    g = idx.make_groups(np.arange(n) % 7)
    assert len(idx.search_collapsed(x[0], 5, groups=g)) == 5
    with pytest.raises(NotImplementedError, match="per-query"):
        idx.search_collapsed_batch(x[:2], 5, groups=g, filter=idx.make_query_filters(np.ones((2, n), bool)))
    with pytest.raises(NotImplementedError, match="per-query"):
        idx._corpus.search_collapsed(x[:2], 5, groups=g, filter=idx.make_query_filters(np.ones((2, n), bool)))
    with pytest.raises(ValueError, match="int8"):
        idx.search_collapsed(x[0], 5, groups=g, approx=True)
    with pytest.raises(ValueError, match="exceeds the pool"):
        idx.search_collapsed(x[0], 50, groups=g, candidates=40)
    assert idx.search_collapsed(x[0], 0, groups=g) == []
    assert idx.search_collapsed(x[0], 5, groups=g, filter=np.zeros(n, bool)) == []
    idx.remove(["d5"])
    with pytest.raises(ValueError, match="another corpus"):
        idx.search_collapsed(x[0], 5, groups=g)
    assert len(idx.search_collapsed(x[0], 5, groups=(np.arange(n - 1) % 7))) == 5


def test_approx_route_equals_the_model_on_the_int8_records():
    from dewi.backends import ExactIndex
    idx, x, cluster, sources, queries = planted(ExactIndex, int8_shadow=True)
    labels = factorised(sources)
    rows, scores, hits = idx.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=sources, per_group=1, candidates=200, approx=True,
                                                    return_hits=True)
    want = model_rows(idx._corpus, queries, labels, 10, 1, 0.3, 0.0, 200, approx=True)
    assert rows.tolist() == want[0].tolist() and bits_equal(scores, want[1]) and hits.tolist() == want[2].tolist()
    mask = np.random.RandomState(3).rand(N_IDX) < 0.5
    rows = idx.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=sources, candidates=200, approx=True, rescore=False, filter=mask)[0]
    assert mask[rows].all() and all(len(set(labels[r].tolist())) == 10 for r in rows)


def test_ivf_and_facade_answer_like_the_exact_index():
    from dewi.backends import ExactIndex
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    exact, x, cluster, sources, queries = planted(ExactIndex)
    ivf = planted(IVFIndex, nlist=16, nprobe=2)[0]
    facade = planted(DewiIndex, use_ann=False, rerank_eta=0.3)[0]
    mask = np.random.RandomState(3).rand(N_IDX) < 0.5
    for filt in (None, mask):
        want = exact.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=sources, per_group=2, candidates=100, filter=filt, return_hits=True)
        got = ivf.search_collapsed_batch(queries, 10, 0.3, 0.0, groups=sources, per_group=2, candidates=100, filter=filt, return_hits=True)
        assert got[0].tolist() == want[0].tolist() and bits_equal(got[1], want[1]) and got[2].tolist() == want[2].tolist()
        res, hits = facade.search_collapsed_batch(queries, 10, groups=sources, per_group=2, candidates=100, filter=filt, return_hits=True)
        assert [[r[0] for r in row] for row in res] == [[f"doc_{i:04d}" for i in row] for row in want[0]]
        assert [[r[1] for r in row] for row in res] == [[float(s) for s in row] for row in want[1]] and hits == want[2].tolist()
    one = facade.search_collapsed(queries[0], 10, groups=sources, per_group=2, candidates=100)
    assert one == facade.search_collapsed_batch(queries[:1], 10, groups=sources, per_group=2, candidates=100)[0]
    assert ivf.search_collapsed(queries[0], 10, 0.3, 0.0, groups=sources, candidates=100) == \
        exact.search_collapsed(queries[0], 10, 0.3, 0.0, groups=sources, candidates=100)


def test_bf16_and_l2_corpora():
    import torch
    from dewi import _engine as eng
    cp, x = gaussian_corpus(4096, 64, 4160)
    labels = (np.arange(4096) // 16).astype(np.int32)               # every exact copy shares its original's group
    q = (x[[0, 160, 1600]] + 0.1 * np.random.RandomState(2).randn(3, 64)).astype(np.float32)
    for corpus in (cp.to_bf16(), eng.DeviceCorpus(cp.emb, cp.dewi32, cp.ent32, space="l2")):
        g = corpus.make_groups(labels)
        ids, sc, hits = corpus.search_collapsed(q, 10, 0.3, 0.2, groups=g, candidates=64)
        want = model_rows(corpus, q, labels, 10, 1, 0.3, 0.2, 64)
        assert ids.tolist() == want[0].tolist() and bits_equal(sc, want[1]) and hits.tolist() == want[2].tolist()
        assert all(len(set(labels[r].tolist())) == 10 for r in ids)
    bf = cp.to_bf16()
    with pytest.raises(NotImplementedError, match="bf16"):
        bf.search_collapsed(q, 10, 0.3, 0.2, groups=bf.make_groups(labels), filter=bf.make_filter(np.ones(4096, bool)))

"""GPU tests of the near-duplicate groups: the union-find kernels at the ABI (no corpus), then ``duplicate_groups_device``,
``duplicate_groups`` and ``dedup_filter`` on small corpora with planted copies and chains.

Contract: the groups are the connected components of the edges; a label is the group's smallest row, so labels, sizes and
representatives are the same bytes whatever the order of the edges or of the threads.  The reference is the NumPy union-find
of tests/groups_model.py.  Index level: the edges are exactly the pairs ``near_duplicates_device`` reports for the same corpus,
and for the cosine fp32 cases also the float64 oracle's pairs (every similarity further than parity.GAP from the threshold).

Shapes: n = 4097 rows (no multiple of 64 or 256, 17 workgroups of 256 edges) and n = 10 007 at the ABI; N = 3000 stored rows
at the index, chunks of 257 (12 union calls, a ragged last one) and 2048 (two).
"""
import ctypes
import functools

import numpy as np
import pytest

import dewi_oracle as orc
import groups_model as gm
from parity import GAP
from test_hip_range_shadow import _DupCase, _clustered, _unit

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- ABI level
class _UnionFind:
    """One workspace on the current device: begin at construction, then unions, then any number of finishes."""

    def __init__(self, n):
        import torch
        from dewi import _native as nat
        self.torch, self.nat, self.lib, self.n = torch, nat, nat.load_library(), n
        need = self.lib.dewi_groups_workspace_bytes(n)
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        nat.check(self.lib.dewi_groups_begin(n, nat.ptr(self.ws), need, nat.stream_ptr()))

    def _dev(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64)).cuda()

    def pairs(self, a, b):
        nat = self.nat
        a, b = self._dev(a), self._dev(b)
        nat.check(self.lib.dewi_groups_union_pairs(self.n, nat.ptr(a), nat.ptr(b), a.numel(), nat.ptr(self.ws), self.ws.numel(),
                                                   nat.stream_ptr()))
        return self

    def lists(self, lims, rows, first_row):
        nat = self.nat
        lims, rows = self._dev(lims), self._dev(rows)
        nat.check(self.lib.dewi_groups_union_lists(self.n, nat.ptr(lims), nat.ptr(rows), lims.numel() - 1, rows.numel(), first_row,
                                                   nat.ptr(self.ws), self.ws.numel(), nat.stream_ptr()))
        return self

    def finish(self, keep=0, key=None, id_offset=0):
        torch, nat = self.torch, self.nat
        out = [torch.full((self.n,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
        k = None if key is None else torch.from_numpy(np.ascontiguousarray(key, dtype=np.float32)).cuda()
        n_groups, bad = ctypes.c_int64(-1), ctypes.c_int64(-1)
        nat.check(self.lib.dewi_groups_finish(self.n, keep, nat.ptr(k), id_offset, nat.ptr(out[0]), nat.ptr(out[1]), nat.ptr(out[2]),
                                              ctypes.byref(n_groups), ctypes.byref(bad), nat.ptr(self.ws), self.ws.numel(),
                                              nat.stream_ptr()))
        return tuple(t.cpu().numpy() for t in out) + (int(n_groups.value), int(bad.value))


def _same(got, want, what=""):
    for name, g, w in zip(("labels", "sizes", "representatives"), got[:3], want[:3]):
        assert g.dtype == np.int64 and np.array_equal(g, w), f"{what}: {name} differ at row {int(np.argmax(g != w))}"
    assert got[3] == want[3], f"{what}: n_groups {got[3]} != {want[3]}"


N1 = 4097


def _one_group(n):
    return (np.zeros(n, np.int64), np.full(n, n, np.int64), np.zeros(n, np.int64), 1)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_path_is_one_group_whatever_the_order_of_its_edges(order):
    a, b = np.arange(N1 - 1), np.arange(1, N1)
    if order == "descending":
        a, b = a[::-1], b[::-1]
    elif order == "shuffled":
        p = np.random.RandomState(0).permutation(N1 - 1)
        flip = np.random.RandomState(1).rand(N1 - 1) < 0.5
        a, b = np.where(flip, b, a)[p], np.where(flip, a, b)[p]
    got = _UnionFind(N1).pairs(a, b).finish()
    _same(got, _one_group(N1), order)
    assert got[4] == 0


def test_stars_repeated_edges_and_self_loops():
    hub = np.full(N1 - 1, N1 - 1)
    _same(_UnionFind(N1).pairs(hub, np.arange(N1 - 1)).finish(), _one_group(N1), "star, hub the highest row")
    # all 4096 edges (i, 0): every thread contends for one root
    _same(_UnionFind(N1).pairs(np.arange(1, N1), np.zeros(N1 - 1, np.int64)).finish(), _one_group(N1), "all edges to row 0")
    # every edge of the path 8 times, plus a self-loop on every row, shuffled
    a = np.concatenate([np.repeat(np.arange(N1 - 1), 8), np.arange(N1)])
    b = np.concatenate([np.repeat(np.arange(1, N1), 8), np.arange(N1)])
    p = np.random.RandomState(2).permutation(a.size)
    _same(_UnionFind(N1).pairs(a[p], b[p]).finish(), _one_group(N1), "repeated edges")
    # self-loops alone join nothing
    got = _UnionFind(N1).pairs(np.arange(N1), np.arange(N1)).finish()
    _same(got, (np.arange(N1), np.ones(N1, np.int64), np.arange(N1), N1), "self-loops")


N2, E2 = 10007, 5000


@functools.lru_cache(maxsize=None)
def _random_graph():
    r = np.random.RandomState(3)
    a, b = r.randint(0, N2, E2), r.randint(0, N2, E2)
    key = r.rand(N2).astype(np.float32)
    return a, b, key, gm.groups(N2, a, b), gm.groups(N2, a, b, keep="dewi", key=key)


def test_random_pairs_equal_the_model_and_are_bit_equal_across_permutations():
    a, b, key, want_first, want_key = _random_graph()
    sizes = want_first[1]
    assert (sizes == 1).sum() > 1000 and sizes.max() > 100 and ((sizes > 1) & (sizes < 10)).any()   # singletons, trees, one large
    runs = []
    for seed in (None, 4, 5):
        p = np.arange(E2) if seed is None else np.random.RandomState(seed).permutation(E2)
        uf = _UnionFind(N2).pairs(a[p], b[p])
        runs.append((uf.finish(), uf.finish(keep=1, key=key)))
        _same(runs[-1][0], want_first, f"keep first, permutation {seed}")
        _same(runs[-1][1], want_key, f"keep key, permutation {seed}")
    for first, by_key in runs[1:]:
        for x, y in zip(first[:3] + by_key[:3], runs[0][0][:3] + runs[0][1][:3]):
            assert x.tobytes() == y.tobytes()


def test_one_union_call_equals_three_calls_over_thirds_and_id_offset_shifts_labels():
    a, b, _, want, _ = _random_graph()
    uf = _UnionFind(N2)
    for lo in range(0, E2, 1667):
        uf.pairs(a[lo:lo + 1667], b[lo:lo + 1667])
    _same(uf.finish(), want, "three calls")
    lab, sizes, reps, n_groups, _ = uf.finish(id_offset=1 << 33)
    _same((lab - (1 << 33), sizes, reps - (1 << 33), n_groups), want, "id_offset")


def test_an_endpoint_out_of_range_is_counted_and_changes_nothing():
    a, b, _, want, _ = _random_graph()
    bad_a = np.array([N2, 5, -1, 1 << 40, 7, N2 + 3])
    bad_b = np.array([5, N2, 7, 9, -(1 << 35), N2 + 3])
    got = _UnionFind(N2).pairs(np.concatenate([a, bad_a]), np.concatenate([b, bad_b])).finish()
    _same(got, want, "bad endpoints")
    assert got[4] == 6
    assert _UnionFind(N2).pairs(a, b).finish()[4] == 0


@pytest.mark.parametrize("n_queries", [1, 257, 2048])
def test_lists_form_equals_the_pairs_form_on_the_filtered_edges(n_queries):
    first_row = 300
    r = np.random.RandomState(10 + n_queries)
    counts = r.randint(0, 6, n_queries)
    counts[r.rand(n_queries) < 0.3] = 0                     # empty queries, runs of them included
    if n_queries == 1:
        counts[:] = 9
    else:
        counts[0] = counts[-1] = 0
        counts[n_queries // 2] = 700                        # one query spans several workgroups of results
    lims = np.zeros(n_queries + 1, np.int64)
    np.cumsum(counts, out=lims[1:])
    q = np.repeat(np.arange(n_queries), counts) + first_row
    rows = r.randint(0, N1, q.size)
    rows[::5] = q[::5]                                      # the query's own row, as the dense route returns it
    rows[1::7] = np.maximum(q[1::7] - 1 - r.randint(0, 300, q[1::7].size), 0)    # rows below the query
    keep = rows > q
    assert keep.any() and (~keep).sum() > q.size // 5
    want = gm.groups(N1, q[keep], rows[keep])
    assert want[3] < N1
    got = _UnionFind(N1).lists(lims, rows, first_row).finish()
    _same(got, want, "lists form")
    assert got[4] == 0
    _same(_UnionFind(N1).pairs(q[keep], rows[keep]).finish(), want, "pairs form")
    # a row past the end is counted, never used
    rows2 = rows.copy()
    hit = int(np.flatnonzero(keep)[0])
    rows2[hit] = N1
    got = _UnionFind(N1).lists(lims, rows2, first_row).finish()
    keep[hit] = False
    _same(got, gm.groups(N1, q[keep], rows[keep]), "lists form, one bad row")
    assert got[4] == 1


def test_keep_max_key_ties_go_to_the_lowest_row_and_nan_never_wins_over_a_number():
    nan = np.float32("nan")
    r = np.random.RandomState(6)
    n = N1
    a, b = np.arange(n - 1), np.arange(1, n)
    cut = (np.arange(n - 1) % 9) != 8                        # groups of 9 consecutive rows (the last one shorter)
    a, b = a[cut], b[cut]
    key = r.randint(0, 3, n).astype(np.float32)              # many ties
    key[r.rand(n) < 0.3] = nan
    key[9:18] = nan                                          # an all-NaN group: its lowest row
    key[18:27] = [nan, -np.inf, nan, -np.inf, nan, nan, nan, nan, nan]      # -inf beats NaN; tie to row 19
    key[27:36] = [-0.0, 0.0, -1.0, nan, -0.0, 0.0, -5.0, nan, -2.0]         # -0 == +0: row 27
    want = gm.groups(n, a, b, keep="dewi", key=key)
    assert want[2][9] == 9 and want[2][18] == 19 and want[2][27] == 27
    got = _UnionFind(n).pairs(a, b).finish(keep=1, key=key)
    _same(got, want, "keep = max key")
    reps = got[2]
    assert np.all(got[0][reps] == got[0])                    # a representative is a member of its group
    shown = np.where(np.isnan(key), -np.inf, key)            # what a key is worth: NaN below every number
    best = np.maximum.reduceat(shown, np.arange(0, n, 9))
    assert np.array_equal(shown[reps], best[np.arange(n) // 9])


# ---------------------------------------------------------------------------------------------------- index level
N3, THR = 3000, 0.9
COS_STEP = 0.95                                              # neighbours on a chain; two steps apart: 2 * 0.95^2 - 1 = 0.805


class _GroupCase:
    """N = 3000 clustered rows with 200 perturbed copies, one group of 40 exact copies scattered through the corpus (both as
    ``_DupCase`` plants them) and 6 chains of 8 unit vectors on a great circle, neighbours at cos = 0.95, rows scattered."""

    def __init__(self, dim, space="cosine", shadow=False, bf16=False):
        from dewi.backends import ExactIndex
        self.dim, self.n, self.space = dim, N3, space
        X, _ = _clustered(N3, dim, 0, noise=1.0, n_queries=8)
        r = np.random.RandomState(1)
        perm = r.permutation(N3)
        dst, src = perm[:200], perm[200:400]
        X[dst] = _unit(X[src] + 0.01 * r.randn(200, dim))
        self.copies = np.sort(perm[400:440])
        X[self.copies] = X[perm[440]]
        self.copies = np.sort(np.append(self.copies, perm[440]))
        theta = np.arccos(COS_STEP)
        self.chains = perm[500:548].reshape(6, 8)
        for rows in self.chains:
            u, w = np.linalg.qr(r.randn(dim, 2))[0].T
            for k, row in enumerate(rows):
                X[row] = (np.cos(k * theta) * u + np.sin(k * theta) * w).astype(np.float32)
        self.X = X
        self.ids = [f"doc_{i:07d}" for i in range(N3)]
        self.cols = orc.synth_payload_columns(N3, seed=0)
        self.index = ExactIndex(dim, space, batch_shadow=shadow)
        self.index.add_batch_columns(self.ids, X, self.cols)
        self.index.build()
        if bf16:
            self.index._corpus = self.index._corpus.to_bf16()
            self.index._host_rows = None
        self.corpus = self.index._corpus
        self.tau = THR if space == "cosine" else -(2.0 - 2.0 * THR)          # -||e - q||^2 of unit rows at cos = 0.9
        self.dewi32 = self.corpus.dewi32.cpu().numpy()
        import torch
        with torch.cuda.device(self.corpus.device):
            a, b, _ = (t.cpu().numpy() for t in self.corpus.near_duplicates_device(self.tau))
        self.pairs = (a, b)
        self.want = {keep: gm.groups(N3, a, b, keep=keep, key=self.dewi32) for keep in ("first", "dewi")}

    def groups(self, **kw):
        import torch
        with torch.cuda.device(self.corpus.device):
            out, n_groups = self.corpus.duplicate_groups_device(self.tau, **kw)
            return tuple(t.cpu().numpy() for t in out) + (n_groups,)


CONFIGS = {
    "shadow-256": dict(dim=256, shadow=True),
    "shadow-384": dict(dim=384, shadow=True),
    "dense-256": dict(dim=256),
    "l2-256": dict(dim=256, space="l2"),
    "bf16-256": dict(dim=256, bf16=True),
    "dense-100": dict(dim=100),
}


@functools.lru_cache(maxsize=None)
def _group_case(name):
    return _GroupCase(**CONFIGS[name])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_duplicate_groups_are_the_components_of_the_near_duplicate_pairs(name):
    case = _group_case(name)
    c = case.corpus
    if name.startswith("shadow"):                            # the chunks below go through the bf16 shadow
        assert c.shadow is not None and 257 >= c.range_shadow_min_batch
        assert c._lib.dewi_knn_range_shadow_supported(c.n_rows, c.dim, 0) == 1
    else:
        assert c.shadow is None
    a, b = case.pairs
    assert a.size >= 200 + 41 * 40 // 2 + 6 * 7
    labels, sizes, _, n_groups = case.want["first"]
    # the planted material: the 41 copies are one group, every chain is one group of 8 (single linkage), nothing else is large
    assert np.all(labels[case.copies] == case.copies[0]) and sizes[case.copies[0]] == 41
    for rows in case.chains:
        assert np.all(labels[rows] == rows.min()) and sizes[rows[0]] == 8
        assert not np.any((a == min(rows[0], rows[2])) & (b == max(rows[0], rows[2])))       # two steps apart: no pair
    assert n_groups < N3 - 200 and np.unique(sizes).tolist() == [1, 2, 8, 41]
    for chunk in (257, 2048):
        for keep in ("first", "dewi"):
            _same(case.groups(chunk=chunk, keep=keep), case.want[keep], f"{name}, chunk {chunk}, keep {keep}")
    if name.startswith("shadow"):
        _same(case.groups(use_shadow=False), case.want["first"], f"{name}, dense route")


@pytest.mark.parametrize("name", ["shadow-256", "shadow-384", "dense-256", "dense-100"])
def test_duplicate_groups_equal_the_components_of_the_float64_oracle_pairs(name):
    case = _group_case(name)
    a64, b64, margin = _DupCase.oracle_pairs(case, THR)
    assert margin > GAP, f"an oracle similarity lies within {margin:.2e} of the threshold"
    want = gm.groups(N3, a64, b64, keep="dewi", key=case.dewi32)
    _same(case.groups(keep="dewi"), want, name)


def test_groups_from_pairs_device_equals_the_model():
    import torch
    case = _group_case("dense-256")
    a, b = case.pairs
    c = case.corpus
    with torch.cuda.device(c.device):
        ta, tb = torch.from_numpy(b).to(c.device), torch.from_numpy(a).to(c.device)         # endpoints swapped: any order
        for keep in ("first", "dewi"):
            out, n_groups = c.groups_from_pairs_device(ta, tb, keep=keep)
            _same(tuple(t.cpu().numpy() for t in out) + (n_groups,), case.want[keep], keep)
        out, n_groups = c.groups_from_pairs_device(ta[:10], tb[:10], n_rows=N3 + 5)
        _same(tuple(t.cpu().numpy() for t in out) + (n_groups,), gm.groups(N3 + 5, a[:10], b[:10]), "n_rows")
        with pytest.raises(ValueError, match="outside"):
            c.groups_from_pairs_device(torch.tensor([0, N3], device=c.device), torch.tensor([1, 2], device=c.device))
        with pytest.raises(ValueError, match="dewi"):
            c.groups_from_pairs_device(ta, tb, n_rows=N3 + 5, keep="dewi")


def test_a_large_cluster_groups_where_the_pairs_exceed_max_pairs():
    from dewi.backends import ExactIndex
    n, m, dim = 2000, 1500, 256
    X, _ = _clustered(n, dim, 0, noise=1.0, n_queries=8)
    rows = np.sort(np.random.RandomState(7).permutation(n)[:m])
    X[rows] = X[rows[0]]
    index = ExactIndex(dim, "cosine", batch_shadow=True)
    index.add_batch_columns([f"d{i}" for i in range(n)], X, orc.synth_payload_columns(n, seed=0))
    assert m * (m - 1) // 2 > 10 ** 6
    with pytest.raises(ValueError, match="max_pairs"):
        index.near_duplicates(THR, max_pairs=10 ** 6)
    g = index.duplicate_groups(THR, keep="first")
    assert np.all(g.labels[rows] == rows[0]) and np.all(g.sizes[rows] == m) and np.all(g.representatives[rows] == rows[0])
    rest = np.setdiff1d(np.arange(n), rows)
    assert np.array_equal(g.labels[rest], rest) and np.all(g.sizes[rest] == 1) and g.n_groups == n - m + 1


def test_dedup_filter_keeps_the_highest_dewi_member_of_every_group():
    case = _group_case("shadow-256")
    index = case.index
    want_labels, _, want_reps, n_groups = case.want["dewi"]
    g = index.duplicate_groups(THR)                                          # keep="dewi" is the default
    _same((g.labels, g.sizes, g.representatives, g.n_groups), case.want["dewi"], "ExactIndex.duplicate_groups")
    for lab in np.unique(want_labels[case.want["dewi"][1] > 1]).tolist():    # the representative: highest dewi, lowest row
        members = np.flatnonzero(want_labels == lab)
        assert g.representatives[lab] == members[np.argmax(case.dewi32[members])]
    flt = index.dedup_filter(THR)
    mask = g.representatives == np.arange(N3)
    assert len(flt) == n_groups == int(mask.sum())
    import torch
    allowed = flt.buf.view(torch.int32)[16:16 + len(flt)].cpu().numpy()      # the prepared list: the allowed rows, ascending
    assert np.array_equal(allowed, np.flatnonzero(mask))
    model = index.make_filter(want_reps == np.arange(N3))
    _, Q = _clustered(N3, case.dim, 0, noise=1.0, n_queries=8)
    Q = np.concatenate([Q, case.X[case.copies[:2]], case.X[case.chains[0][3:5]]])      # queries that sit inside groups
    rows, scores = index.search_batch(Q, 10, filter=flt)
    rows_m, scores_m = index.search_batch(Q, 10, filter=model)
    assert np.array_equal(rows, rows_m) and scores.tobytes() == scores_m.tobytes()
    assert np.all(mask[rows])
    for rr in rows:
        assert np.unique(g.labels[rr]).size == rr.size                       # no two results of a query share a group
    plain, _ = index.search_batch(Q, 10)
    assert any(np.unique(g.labels[rr]).size < rr.size for rr in plain)       # ... which the unfiltered search does not give


def test_dedup_filter_of_a_bf16_corpus_is_not_served():
    case = _group_case("bf16-256")
    with pytest.raises(NotImplementedError):
        case.index.dedup_filter(case.tau)


def test_dewi_index_clusters_partition_the_ids_in_label_and_row_order():
    from dewi.index import DewiIndex
    from dewi.types import payloads_from_columns
    n, dim = 600, 64
    X, _ = _clustered(n, dim, 0, noise=1.0, n_queries=8)
    r = np.random.RandomState(8)
    perm = r.permutation(n)
    X[perm[:60]] = _unit(X[perm[60:120]] + 0.01 * r.randn(60, dim))
    X[perm[120:130]] = X[perm[130]]
    ids = [f"doc_{i:05d}" for i in range(n)]
    index = DewiIndex(dim=dim, use_ann=False)
    index.add_batch(ids, X, payloads_from_columns(orc.synth_payload_columns(n, seed=0)))
    g = index.duplicate_groups(THR, doc_ids=True)
    assert index._built
    assert sorted(x for c in g.clusters for x in c) == ids and len(g.clusters) == g.n_groups       # a partition of all ids
    assert sum(len(c) == 1 for c in g.clusters) >= n - 140                                          # singletons included
    firsts = [ids.index(c[0]) for c in g.clusters]
    assert firsts == sorted(firsts) and np.array_equal(np.unique(g.labels), firsts)                # ordered by label
    for c in g.clusters:
        rows = [ids.index(x) for x in c]
        assert rows == sorted(rows) and np.all(g.labels[rows] == rows[0]) and np.all(g.sizes[rows] == len(c))
    assert max(len(c) for c in g.clusters) == 11
    a, b, _ = index.near_duplicates(THR)
    _same((g.labels, g.sizes, g.representatives, g.n_groups),
          gm.groups(n, a, b, keep="dewi", key=index._backend._corpus.dewi32.cpu().numpy()), "DewiIndex")
    flt = index.dedup_filter(THR)
    assert len(flt) == g.n_groups

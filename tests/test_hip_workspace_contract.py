"""GPU tests of the workspace contract (include/dewi_hip.h): a workspace's contents on entry are undefined, and no call reads
or writes outside ``[d_workspace, d_workspace + workspace_bytes)`` or outside its declared outputs.

Every case is one (route, pattern) and runs the same four steps (tests/wsguard.py holds the guards):

  1. the corpus of the route (built once per route, module-level cache), every cached workspace dropped, one warm call:
     the caches are filled by THIS call alone, and its result is the base;
  2. the base result against the oracle, once per route (``parity.check_batch``; range, groups and the fit against a float64
     / NumPy reference of their own definition) — without this anchor two equal wrong answers would pass;
  3. ``guard`` + ``poison(pattern)`` on every owner of a workspace, the same call into guarded outputs: every result tensor
     (ids, scores, records, lims, counts, labels, ``refused_by_last_call()``) is BIT-equal to the base, ``check()`` passes (guards
     untouched, the cache still holds the guarded view, the interior was written), the guard rows of the outputs are
     untouched and every output slot was written;
  4. the same call once more on its own leftovers, one call of another batch size and k on the same object, then the
     original call again: still bit-equal; the guards are still intact.  Every route has such a second shape (``other()``;
     the base class raises).  ``pipelined-depth3`` is the one whose second shape cannot run in the SAME workspaces: a
     ``PipelinedSearcher`` is built for one batch size, k and cut and owns its slots, so the other shapes there are a plain
     search and a second pipeline of another k on the same corpus.

The patterns run from mild to hostile (zeros, random bytes, 0x7F, 0xFF), so a logic error shows as a mismatch before a count
of 2^32 - 1 could be read as a loop bound.  Each route asserts the path the library takes for it (``scan_kernel_name``, a
``dewi_knn_refusal_flags`` offset, ``dewi_knn_range_shadow_supported``, a workspace size that is not 0).

DECISIVE COUNTS of the anchors (``parity.count_decisive`` on the CPU, the oracle alone; bf16 with the oracle's own
``bf16_round(prepare_query)``): rows fp32, 3001 rows (1500 at dim 4100), 5 queries, seed = dim — k = 10: 5/5 at every dim;
k = 40: 5/5; k = 150: 5/5 (dim 100: 4/5) -> floors 0.8 / 0.8 / 0.6 (tests/test_hip_odd_rows.py: 0.8 at k <= 10 and 0.6 above
for the same generator).  k = 1025: 0/5 at every dim but 100 (1/5), and no blend weights change that — 1026 adjusted scores
inside an interval of ~0.3 always hold a pair closer than GAP — so that route is anchored by ``compare_query``'s near-tie rules
for every query (every id an admissible candidate, every score the oracle's blend for THAT row, no sure candidate left out,
no duplicates, descending) without a decisive floor.  bf16 rows: 5/5, 5/5, 5/5 (dim 1000: 4/5), 0/5 at gap 1e-6: the same.
Matrix-core routes, 65 600 rows, seed = dim + b, k = 10: 8/8, 33/33, 8/8 (dim 200), 5/5 (l2), 40/40, bf16 8/8 and 40/40 ->
floor 0.75 as tests/test_hip_mfma.py; the one query of the list route: 1/1.  Merge of three shards: k = 10 5/5, k = 350 2/5
-> floors 0.8, 0.4.  Planted runs: floor 0.75, the condition tests/test_corpora_host.py checks.  Filters, IVF, range: their
own tests' floors (half, 0.8, 0.8 of the queries).

NOT covered here: ``dewi_diverse_rerank`` — ``dewi_diverse_workspace_bytes(...) == 0`` for every shape it takes
(tests/test_diverse_host.py pins that), so it has no workspace to poison; its outputs are guarded in ``search-diverse``.
"""
import ctypes

import numpy as np
import pytest

import corpora
import dewi_oracle as orc
import groups_model as gm
import wsguard as wsg
from parity import GAP, SCORE_TOL, check_batch, compare_query, device_prepared_queries

pytestmark = pytest.mark.gpu

ETA, PREF = 0.3, 0.1
TOL_BF16 = dict(gap=1e-6, score_tol=1e-5, prepared=True, exact_gaps=False)
NO_FLAGS = ctypes.c_size_t(-1).value

_corpora = {}         # key -> built corpus + host data: one per shape, shared by the routes and patterns that use it
_routes = {}          # route name -> Route (its base result is anchored to the oracle once)


def _torch():
    import torch
    return torch


def _eng():
    from dewi import _engine
    return _engine


def _nat():
    from dewi import _native
    return _native


def _host(result):
    """A result tuple as host copies (the device tensors may be reused by the next call)."""
    torch = _torch()
    return tuple(t.detach().cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t) for t in result)


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _clustered(n, d, seed, noise=1.0, n_queries=64, n_centres=64):
    r = np.random.RandomState(seed)
    cen = r.randn(n_centres, d)
    lab = r.randint(0, n_centres, n)
    X = _unit(cen[lab] + noise * r.randn(n, d))
    rows = r.choice(n, n_queries, replace=False)
    return X, _unit(X[rows] + 0.05 * r.randn(n_queries, d))


class _Data:
    """A device corpus with the oracle's view of it."""

    def __init__(self, raw, cols, Q, kind="f32", space="cosine", single_query=False, id_offset=0):
        eng = _eng()
        c = eng.DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space=space, id_offset=id_offset)
        if kind == "bf16":
            c = c.to_bf16()
        if kind == "shadow":
            c.enable_bf16_shadow(single_query=single_query)
        self.c, self.kind, self.space, self.Q = c, kind, space, np.ascontiguousarray(Q, dtype=np.float32)
        self.E = (c.emb.float() if c.is_bf16 else c.emb).cpu().numpy()
        self.dewi32, self.ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
        self.q_dev = _torch().from_numpy(self.Q).cuda()
        self._qp = None

    def oracle_queries(self):
        if self.kind != "bf16":
            return self.Q, {}
        if self._qp is None:
            self._qp = device_prepared_queries(self.Q, self.space)
        return self._qp, TOL_BF16


def _synth(n, dim, b, kind="f32", space="cosine", seed=None, **kw):
    key = ("synth", n, dim, b, kind, space, seed, tuple(sorted(kw.items())))
    if key not in _corpora:
        seed_ = dim if seed is None else seed
        raw = orc.synth_corpus(n, dim, seed=seed_)
        Q = orc.synth_queries(b, dim, seed=seed_ + 1)
        if space == "l2":                                  # (rows and queries of comparable norm: distances that differ)
            rng = np.random.default_rng(seed_)
            raw = raw * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
            Q = Q * rng.uniform(0.5, 2.0, size=(b, 1)).astype(np.float32)
        _corpora[key] = _Data(raw, orc.synth_payload_columns(n, seed=seed_), Q, kind, space, **kw)
    return _corpora[key]


def _owners_of_filter_pass(n):
    cus = ctypes.c_int(0)
    _nat().check(_nat().load_library().dewi_device_info(ctypes.byref(cus), None, None))
    return min((n + corpora.TILE_ROWS - 1) // corpora.TILE_ROWS, int(cus.value))


def _planted(case, kind):
    key = ("planted", case, kind)
    if key not in _corpora:
        n, dim, b, k, d_max = corpora.PLANTED_CASES[case]
        X, Q, D, _ = corpora.planted_runs(n, dim, b, seed=dim + b, d_max=d_max, owners=_owners_of_filter_pass(n))
        _corpora[key] = _Data(X, orc.synth_payload_columns(n, seed=dim + b), Q, kind, single_query=True)
    return _corpora[key]


# ====================================================================================================== routes
class Route:
    """One entry point on one shape.  ``call(guarded)`` -> (result tuple, [GuardedOutput]); ``other()``: a call of another
    batch size and k on the same object; ``owners()``: everything whose cached workspaces the call uses (after a warm call);
    ``reset()``: drop those caches; ``anchor(host result)``: the base against the oracle; ``assert_route()``."""

    base = None

    def reset(self):
        for o in self.corpora():
            o.drop_cached_workspaces()

    def corpora(self):
        return []

    def owners(self):
        return self.corpora()

    def assert_route(self):
        pass

    def other(self):
        raise NotImplementedError("every route makes one call of another batch size and k on the same object (step 4)")

    def after(self, result):
        """Per-call assertions beyond bit-equality (ids in range, flags)."""


def _flags_offset(c, through_shadow, b, k, cut):
    off = ctypes.c_size_t(0)
    nat = _nat()
    nat.check(c._lib.dewi_knn_refusal_flags(c._elem, 1 if through_shadow else 0, c.n_rows, c.dim, b, k, cut, nat.SPACE_CODES[c.space],
                                            ctypes.byref(off)))
    return off.value


class Search(Route):
    """``search_device`` (ids, scores, refusal flags)."""

    def __init__(self, data, k, prefix=None, floor=0.8, flags=None, refused=None, other=(3, 7), eta=ETA, pref=PREF, b=None,
                 shadow_kernel=None):
        self.d, self.k, self.prefix, self.floor, self.flags, self.refused, self._other = data, k, prefix, floor, flags, refused, other
        self.shadow_kernel = shadow_kernel                   # shadow corpora: the pass over the bf16 copy
        self.eta, self.pref = eta, pref
        self.b = data.Q.shape[0] if b is None else b
        self.q = data.q_dev[: self.b].contiguous()

    def corpora(self):
        return [self.d.c]

    def assert_route(self):
        c = self.d.c
        cut = min(2 * self.k, c.n_rows)
        if self.prefix is not None:
            name = c.scan_kernel_name(self.b, self.k)
            assert name.startswith(self.prefix), (name, self.prefix)
        shadow = self.d.kind == "shadow"
        if shadow:
            # the warm call really took dewi_knn_rerank_f32_shadow, and the pass over the bf16 copy is the one this route is
            # about: the library names the kernel a bf16 matrix of this shape and batch takes (plan_shadow asks the same
            # mfma_path_supported / mfma_f32_path_supported; the list route's scan is the one-query bf16 row kernel)
            assert c._last_call[3] is True and c.shadow is not None and c.shadow.shape == c.emb.shape
            assert self.shadow_kernel is not None
            buf = ctypes.create_string_buffer(128)
            _nat().check(c._lib.dewi_knn_scan_kernel(1, c.n_rows, c.dim, self.b, cut, _nat().SPACE_CODES[c.space], buf, 128))
            assert buf.value.decode().startswith(self.shadow_kernel), (buf.value.decode(), self.shadow_kernel)
            if self.b == 1:                                  # the list route: one query, a cut of at most 32, at least 64 K rows
                assert c.shadow_min_batch == 1 and cut <= 32 and c.n_rows >= 64 * 1024
        else:
            assert c._last_call[3] is False
        off = _flags_offset(c, shadow, self.b, self.k, cut)
        if self.flags:
            assert off != NO_FLAGS, "this shape does not take a matrix-core pass: no refusal flags"
            assert off % 4 == 0 and off + 4 * self.b <= c.cached_workspaces()[(self.b, cut)].numel()
        elif self.flags is False:
            assert off == NO_FLAGS, "a row-kernel route with refusal flags"

    def call(self, guarded):
        c, outs = self.d.c, []
        if guarded:
            outs = [wsg.GuardedOutput((self.b, self.k), _torch().int64, c.device, label="out_ids"),
                    wsg.GuardedOutput((self.b, self.k), _torch().float32, c.device, label="out_scores")]
            ids, sc = c.search_device(self.q, self.k, self.eta, self.pref, outs[0].mid, outs[1].mid)
        else:
            ids, sc = c.search_device(self.q, self.k, self.eta, self.pref)
        return (ids, sc, c.refused_by_last_call()), outs

    def other(self):
        ob, ok = self._other
        q = self.q[:ob].contiguous() if self.b >= ob else self.q[:1].repeat(ob, 1)
        ids, _ = self.d.c.search_device(q, ok, self.eta, self.pref)
        assert ids.min().item() >= 0

    def after(self, result):
        ids, sc, refused = result
        wsg.check_ids(ids, self.d.c.n_rows)
        if self.refused is False:
            assert not refused.any(), "an ordinary batch: every flag must read 0"
        elif self.refused:
            assert refused.any() and not refused.all(), "the batch must mix refused and served queries"

    def anchor(self, result):
        ids, sc, _ = result
        Qo, tol = self.d.oracle_queries()
        kw = dict(tol)
        if self.d.c.n_rows > 10000:
            kw["exact_gaps"] = False
        if self.floor is None:                             # (k = 1025: no query is decisive on the oracle, see the module docstring)
            for j in range(self.b):
                _, msg = compare_query(self.d.E, Qo[j], self.d.dewi32, self.d.ent32, self.k, self.eta, self.pref, self.d.space,
                                       ids[j], sc[j], **kw)
                assert msg is None, f"query {j}: {msg}"
            return
        check_batch(self.d.E, Qo[: self.b], self.d.dewi32, self.d.ent32, self.k, self.eta, self.pref, self.d.space, ids, sc,
                    min_decisive_frac=self.floor, **kw)


class Filtered(Route):
    """``search_device(filter=DeviceFilter)``: the list is shorter than the cut (``short``) or longer."""

    def __init__(self, data, mask, k):
        self.d, self.k, self.rows = data, k, np.flatnonzero(mask)
        self.f = data.c.make_filter(mask)
        self.b = data.Q.shape[0]

    def corpora(self):
        return [self.d.c]

    def assert_route(self):
        c = self.d.c
        cut = min(2 * self.k, self.rows.size)
        assert ("filtered", self.b, self.rows.size, cut) in c.cached_workspaces()

    def call(self, guarded):
        c, outs = self.d.c, []
        if guarded:
            outs = [wsg.GuardedOutput((self.b, self.k), _torch().int64, c.device, label="out_ids"),
                    wsg.GuardedOutput((self.b, self.k), _torch().float32, c.device, label="out_scores")]
            res = c.search_device(self.d.q_dev, self.k, ETA, 0.0, outs[0].mid, outs[1].mid, filter=self.f)
        else:
            res = c.search_device(self.d.q_dev, self.k, ETA, 0.0, filter=self.f)
        return tuple(res), outs

    def other(self):
        self.d.c.search_device(self.d.q_dev[:3].contiguous(), min(4, self.rows.size), ETA, 0.0, filter=self.f)

    def after(self, result):
        assert np.isin(result[0], self.rows).all(), "an id outside the filter"

    def anchor(self, result):
        ids, sc = result
        pos = np.searchsorted(self.rows, ids)
        dec = 0
        for j in range(self.b):
            decisive, msg = compare_query(self.d.E[self.rows], self.d.Q[j], self.d.dewi32[self.rows], self.d.ent32[self.rows], self.k,
                                          ETA, 0.0, "cosine", pos[j], sc[j])
            assert msg is None, f"query {j}: {msg}"
            dec += int(decisive)
        assert 2 * dec >= self.b, f"only {dec}/{self.b} decisive queries"


class QueryFiltered(Route):
    """Per-query lists: |F_j| >= c, 0 < |F_j| < c and an empty list in one batch."""

    def __init__(self, data, masks, k):
        self.d, self.k, self.masks = data, k, masks
        self.qf = data.c.make_query_filters(masks)
        self.b = masks.shape[0]
        self.q = data.q_dev[: self.b].contiguous()
        self.other_rows = [0, 1, 4]                          # another batch size and k: |F| ~ 900, 13 (8 <= 13 < 16: on its own), 3001
        self.qf_other = data.c.make_query_filters(masks[self.other_rows])
        self.q_other = data.q_dev[self.other_rows].contiguous()

    def corpora(self):
        return [self.d.c]

    def assert_route(self):
        sizes = self.masks.sum(axis=1)
        c = 2 * self.k
        assert (sizes >= c).sum() >= 2 and ((sizes > 0) & (sizes < c)).any() and (sizes == 0).any()
        keys = list(self.d.c.cached_workspaces())
        assert any(k[0] == "qfiltered" for k in keys) and any(k[0] == "filtered" for k in keys), keys

    def call(self, guarded):
        c, outs = self.d.c, []
        if guarded:
            outs = [wsg.GuardedOutput((self.b, self.k), _torch().int64, c.device, label="out_ids"),
                    wsg.GuardedOutput((self.b, self.k), _torch().float32, c.device, label="out_scores")]
            res = c.search_device(self.q, self.k, ETA, 0.0, outs[0].mid, outs[1].mid, filter=self.qf)
        else:
            res = c.search_device(self.q, self.k, ETA, 0.0, filter=self.qf)
        return tuple(res), outs

    def other(self):
        c = self.d.c
        before = set(c.cached_workspaces())
        ids, _ = c.search_device(self.q_other, 8, ETA, 0.0, filter=self.qf_other)
        # a "qfiltered" workspace of its own next to the route's; its 13-row list runs with k = 8 in the SAME one-list
        # workspace the route's 13-row list uses with k = 10 (the key holds the batch, the list length and the cut: 1, 13, 13)
        new = set(c.cached_workspaces()) - before
        assert {k[0] for k in new} == {"qfiltered"} and ("filtered", 1, 13, 13) in before, (new, before)
        for j, row in enumerate(self.other_rows):
            assert self.masks[row][ids[j].cpu().numpy()].all(), f"query {j} of the other shape: an id outside its list"

    def after(self, result):
        ids, sc = result
        wsg.check_ids(ids, self.d.c.n_rows, allow_empty=True)
        for j in range(self.b):
            n_j = int(self.masks[j].sum())
            if n_j == 0:
                assert (ids[j] == -1).all() and np.isnan(sc[j]).all(), f"query {j}: an empty list gives id -1 / score NaN"
            else:
                assert self.masks[j][ids[j]].all(), f"query {j}: an id outside its list"

    def anchor(self, result):
        ids, sc = result
        dec = tot = 0
        for j in range(self.b):
            rows = np.flatnonzero(self.masks[j])
            if rows.size == 0:
                continue
            decisive, msg = compare_query(self.d.E[rows], self.d.Q[j], self.d.dewi32[rows], self.d.ent32[rows], self.k, ETA, 0.0,
                                          "cosine", np.searchsorted(rows, ids[j]), sc[j])
            assert msg is None, f"query {j}: {msg}"
            dec, tot = dec + int(decisive), tot + 1
        assert 2 * dec >= tot, f"only {dec}/{tot} decisive queries"


class ShardsAndMerge(Route):
    """``candidates_device`` on three ragged shards (views of one matrix), then ``merge_rerank_device``."""

    def __init__(self, data, cuts, c, k, floor, large):
        eng = _eng()
        self.d, self.c, self.k, self.floor, self.large = data, c, k, floor, large
        w = data.c
        self.shards = [eng.DeviceCorpus(w.emb[lo:hi], w.dewi32[lo:hi], w.ent32[lo:hi], "cosine", id_offset=lo)
                       for lo, hi in zip(cuts[:-1], cuts[1:])]
        self.b = data.Q.shape[0]

    def corpora(self):
        return self.shards

    def reset(self):
        Route.reset(self)
        _eng()._merge_ws.clear()

    def owners(self):
        return self.shards + ([_eng()._merge_ws] if self.large else [])

    def assert_route(self):
        lib = _nat().load_library()
        need = int(lib.dewi_merge_workspace_bytes(len(self.shards), self.b, self.c, self.c))
        assert (need > 0) == self.large and (len(self.shards) * self.c > 2048) == self.large
        assert len(_eng()._merge_ws) == (1 if self.large else 0)

    def call(self, guarded):
        torch, eng = _torch(), _eng()
        dev = self.d.c.device
        n_l = len(self.shards)
        outs = []
        if guarded:
            recs = wsg.GuardedOutput((n_l * self.b, self.c, 4), torch.int32, dev, label="records")
            o_i = wsg.GuardedOutput((self.b, self.k), torch.int64, dev, label="out_ids")
            o_s = wsg.GuardedOutput((self.b, self.k), torch.float32, dev, label="out_scores")
            outs = [recs, o_i, o_s]
            lists = recs.mid.view(n_l, self.b, self.c, 4)
            for s, sh in enumerate(self.shards):
                sh.candidates_device(self.d.q_dev, self.c, out=lists[s])
            ids, sc = eng.merge_rerank_device(lists, self.c, self.k, ETA, PREF, o_i.mid, o_s.mid)
        else:
            lists = torch.stack([sh.candidates_device(self.d.q_dev, self.c) for sh in self.shards])
            ids, sc = eng.merge_rerank_device(lists, self.c, self.k, ETA, PREF)
        return (lists, ids, sc), outs

    def other(self):
        torch = _torch()
        lists = torch.stack([sh.candidates_device(self.d.q_dev[:2].contiguous(), 6) for sh in self.shards])
        _eng().merge_rerank_device(lists, 6, 3, ETA, PREF)

    def after(self, result):
        wsg.check_ids(result[1], self.d.c.n_rows)
        wsg.check_ids(result[0][..., 3], self.d.c.n_rows, allow_empty=True)       # (-1: the padding of a shard with fewer rows than c)
        for s, sh in enumerate(self.shards):
            real = result[0][s, :, : min(self.c, sh.n_rows), 3]
            assert real.min() >= sh.id_offset and real.max() < sh.id_offset + sh.n_rows, f"shard {s}: a record outside its rows"

    def anchor(self, result):
        _, ids, sc = result
        assert self.c == 2 * self.k                        # the oracle's own cut
        check_batch(self.d.E, self.d.Q, self.d.dewi32, self.d.ent32, self.k, ETA, PREF, "cosine", ids, sc, min_decisive_frac=self.floor)


class Pipelined(Route):
    """``PipelinedSearcher`` with three workspaces in rotation, every slot poisoned: four submits (slot 0 twice)."""

    def __init__(self, data, k):
        self.d, self.k = data, k
        self.b = data.Q.shape[0]
        self.pipe = None

    def reset(self):
        self.pipe = _eng().PipelinedSearcher(self.d.c, self.k, ETA, PREF, n_queries=self.b, depth=3)

    def owners(self):
        return [self.pipe]

    def assert_route(self):
        assert self.pipe.depth == 3 and len(self.pipe._ws) == 3
        assert self.d.c.scan_kernel_name(self.b, self.k).startswith("mfma_scan_f32<false")

    def call(self, guarded):
        torch = _torch()
        dev = self.d.c.device
        o_i = wsg.GuardedOutput((4 * self.b, self.k), torch.int64, dev, label="out_ids")
        o_s = wsg.GuardedOutput((4 * self.b, self.k), torch.float32, dev, label="out_scores")
        ids, sc = o_i.mid.view(4, self.b, self.k), o_s.mid.view(4, self.b, self.k)
        torch.cuda.synchronize()                             # the prefill ran on the current stream, the pipeline has its own
        for i in range(4):
            self.pipe.submit(self.d.q_dev, ids[i], sc[i])
        self.pipe.drain()
        return (ids, sc), [o_i, o_s]

    def other(self):
        # A PipelinedSearcher has ONE shape (batch, k and cut are fixed when it is built) and its slots are its own: no call of
        # another shape can run in them.  What another shape can share with it is the corpus and the device: a plain search of
        # 3 queries, k = 4 on its corpus (a row-kernel shape), and a second pipeline of another k on the same corpus, run in
        # between.
        torch, c = _torch(), self.d.c
        ids, _ = c.search_device(self.d.q_dev[:3].contiguous(), 4, ETA, PREF)
        assert ids.min().item() >= 0
        pipe2 = _eng().PipelinedSearcher(c, 3, ETA, PREF, n_queries=self.b, depth=2)
        o_i = torch.empty((self.b, 3), dtype=torch.int64, device=c.device)
        o_s = torch.empty((self.b, 3), dtype=torch.float32, device=c.device)
        torch.cuda.synchronize()
        pipe2.submit(self.d.q_dev, o_i, o_s)
        pipe2.drain()
        assert o_i.min().item() >= 0

    def after(self, result):
        ids, sc = result
        wsg.check_ids(ids, self.d.c.n_rows)
        for i in range(1, 4):
            assert np.array_equal(ids[i], ids[0]) and np.array_equal(sc[i].view(np.uint32), sc[0].view(np.uint32)), f"submit {i}"

    def anchor(self, result):
        ids, sc = result
        check_batch(self.d.E, self.d.Q, self.d.dewi32, self.d.ent32, self.k, ETA, PREF, "cosine", ids[0], sc[0],
                    min_decisive_frac=0.75, exact_gaps=False)


class Diverse(Route):
    """``search_diverse_device``: the candidate scan's workspace is the corpus's; the re-rank itself has none (size 0)."""

    def __init__(self, data, k):
        self.d, self.k = data, k
        self.b = data.Q.shape[0]

    def corpora(self):
        return [self.d.c]

    def assert_route(self):
        assert int(self.d.c._lib.dewi_diverse_workspace_bytes(self.b, 4 * self.k, self.d.c.dim)) == 0

    def call(self, guarded):
        c, outs = self.d.c, []
        if guarded:
            outs = [wsg.GuardedOutput((self.b, self.k), _torch().int64, c.device, label="out_ids"),
                    wsg.GuardedOutput((self.b, self.k), _torch().float32, c.device, label="out_scores")]
            res = c.search_diverse_device(self.d.q_dev, self.k, ETA, 0.0, 1.0, out_ids=outs[0].mid, out_scores=outs[1].mid)
        else:
            res = c.search_diverse_device(self.d.q_dev, self.k, ETA, 0.0, 1.0)
        return tuple(res), outs

    def other(self):
        c = self.d.c
        ids, _ = c.search_diverse_device(self.d.q_dev[:3].contiguous(), 4, ETA, 0.0, 0.5)
        assert (3, 16) in c.cached_workspaces() and ids.shape == (3, 4) and ids.min().item() >= 0

    def after(self, result):
        wsg.check_ids(result[0], self.d.c.n_rows)

    def anchor(self, result):
        # mmr_lambda = 1 without max_sim is the plain search over the pool of 4k candidates: the k best adjusted scores of the
        # float64 pool
        ids, sc = result
        s64 = self.d.Q.astype(np.float64) @ self.d.E.astype(np.float64).T / np.linalg.norm(self.d.Q.astype(np.float64), axis=1)[:, None]
        for j in range(self.b):
            pool = np.argsort(-s64[j], kind="stable")[: 4 * self.k]
            adj = (1 - ETA) * s64[j, pool] + ETA * self.d.dewi32[pool].astype(np.float64)
            want = np.sort(adj)[::-1][: self.k]
            assert np.max(np.abs(sc[j].astype(np.float64) - want)) <= SCORE_TOL, f"query {j}"


class Range(Route):
    """``range_search_routed``: (lims, rows, sims, scores); ``collect`` additionally drives count + collect through the ABI
    with guarded record outputs (one chunk)."""

    def __init__(self, data, b, tau, shadow):
        self.d, self.b, self.tau, self.shadow = data, b, tau, shadow
        self.q = data.q_dev[:b].contiguous()

    def corpora(self):
        return [self.d.c]

    def assert_route(self):
        c, nat = self.d.c, _nat()
        keys = [k[0] for k in c.cached_workspaces()]
        supported = bool(c._lib.dewi_knn_range_shadow_supported(c.n_rows, c.dim, nat.SPACE_CODES[c.space]))
        if self.shadow:
            assert supported and c.shadow is not None and self.b >= c.range_shadow_min_batch and "range_shadow" in keys, keys
        else:
            assert keys and all(k == "range" for k in keys), keys
            n_chunks = (self.b + nat.RANGE_MAX_QUERIES - 1) // nat.RANGE_MAX_QUERIES
            assert len(keys) == min(n_chunks, 2) and (n_chunks == 1 or self.b % nat.RANGE_MAX_QUERIES != 0)

    def call(self, guarded):
        c = self.d.c
        res = c.range_search_routed(self.q, self.tau, ETA, PREF, use_shadow=self.shadow)
        outs = []
        if guarded and not self.shadow and self.b <= _nat().RANGE_MAX_QUERIES:
            outs = self._collect_through_the_abi(res)
        return tuple(res), outs

    def _collect_through_the_abi(self, res):
        """Count + collect of the one chunk once more, into guarded outputs: the rows in ascending order per query."""
        torch, nat, c = _torch(), _nat(), self.d.c
        lims = res[0]
        t_c = int(lims[-1].item())
        ws = c.cached_workspaces()[("range", self.b, c.n_rows)]
        thr = c.stage_thresholds(self.tau, self.b)
        counts = wsg.GuardedOutput((self.b,), torch.int64, c.device, label="range counts")
        nat.check(c._lib.dewi_knn_range_count(nat.ptr(c.emb), c._elem, c.n_rows, c.dim, None, 0, nat.ptr(self.q), self.b, nat.ptr(thr),
                                              nat.SPACE_CODES[c.space], nat.ptr(counts.mid), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        assert torch.equal(counts.mid, lims[1:] - lims[:-1])
        rows = wsg.GuardedOutput((t_c,), torch.int64, c.device, label="range rows")
        sims = wsg.GuardedOutput((t_c,), torch.float32, c.device, label="range sims")
        scores = wsg.GuardedOutput((t_c,), torch.float32, c.device, label="range scores")
        nat.check(c._lib.dewi_knn_range_collect(nat.ptr(ws), ws.numel(), c.n_rows, self.b, nat.ptr(thr), nat.ptr(lims), t_c,
                                                nat.ptr(c.dewi32), nat.ptr(c.ent32), float(ETA), float(PREF), nat.ptr(rows.mid),
                                                nat.ptr(sims.mid), nat.ptr(scores.mid), nat.stream_ptr()))
        torch.cuda.synchronize()
        l, r = lims.cpu().numpy(), rows.mid.cpu().numpy()
        for j in range(self.b):
            assert np.array_equal(r[l[j]:l[j + 1]], np.sort(res[1][l[j]:l[j + 1]].cpu().numpy())), f"query {j}"
        return [counts, rows, sims, scores]

    def other(self):
        self.d.c.range_search_routed(self.d.q_dev[:3].contiguous(), self.tau, ETA, 0.0, use_shadow=False)

    def after(self, result):
        wsg.check_ids(result[1], self.d.c.n_rows)

    def anchor(self, result):
        lims, rows, sims, scores = result
        E64 = self.d.E.astype(np.float64)
        Q64 = np.stack([orc.prepare_query(q, "cosine") for q in self.d.Q[: self.b]]).astype(np.float64)
        s64 = Q64 @ E64.T
        assert lims[0] == 0 and lims[-1] == rows.size and rows.size > self.b, "the threshold must let rows pass"
        dec = 0
        for j in range(self.b):
            r = rows[lims[j]:lims[j + 1]]
            got = np.zeros(E64.shape[0], dtype=bool)
            got[r] = True
            assert got.sum() == r.size, f"query {j}: duplicate rows"
            sure_in, sure_out = s64[j] >= self.tau + GAP, s64[j] < self.tau - GAP
            assert not np.any(sure_in & ~got) and not np.any(sure_out & got), f"query {j}: the set differs from the oracle's"
            dec += int(not np.any(~sure_in & ~sure_out))
            if r.size:
                sm = sims[lims[j]:lims[j + 1]]
                assert np.max(np.abs(sm - s64[j, r])) <= SCORE_TOL, f"query {j}: similarities"
                want = np.float64(np.float32(1 - ETA)) * s64[j, r] + np.float64(np.float32(ETA)) * self.d.dewi32[r] \
                    + np.float64(np.float32(PREF)) * self.d.ent32[r]
                assert np.max(np.abs(scores[lims[j]:lims[j + 1]] - want)) <= SCORE_TOL, f"query {j}: adjusted scores"
        assert dec >= 0.8 * self.b, f"only {dec}/{self.b} decisive queries"


class Duplicates(Route):
    """``near_duplicates_device`` / ``duplicate_groups_device`` / ``groups_from_pairs_device`` on rows with planted copies."""

    THR = 0.9

    def __init__(self, data, which):
        self.d, self.which = data, which
        self.pairs = None

    def corpora(self):
        return [self.d.c]

    def assert_route(self):
        keys = list(self.d.c.cached_workspaces())
        n = self.d.c.n_rows
        if self.which != "pairs":
            assert ("groups", n) in keys, keys
        if self.which != "from_pairs":
            want = "range_shadow" if self.d.c.shadow is not None else "range"
            assert any(k[0] == want for k in keys), keys

    def _oracle_pairs(self):
        X = self.d.E.astype(np.float64)
        S = np.triu(X @ X.T, 1)
        assert np.min(np.abs(S[S != 0] - self.THR)) > GAP, "an oracle similarity lies within GAP of the threshold"
        return np.nonzero(S >= self.THR)

    def call(self, guarded):
        c = self.d.c
        if self.which == "pairs":
            return tuple(c.near_duplicates_device(self.THR, chunk=1024)), []
        if self.which == "groups":
            out, n_groups = c.duplicate_groups_device(self.THR, chunk=1024, keep="dewi")
            return tuple(out) + (np.int64(n_groups),), []
        if self.pairs is None:
            a, b = self._oracle_pairs()
            self.pairs = tuple(_torch().from_numpy(x.astype(np.int64)).to(c.device) for x in (b, a))     # endpoints swapped
        out, n_groups = c.groups_from_pairs_device(*self.pairs, keep="dewi")
        return tuple(out) + (np.int64(n_groups),), []

    def other(self):
        c = self.d.c
        if self.which == "from_pairs":
            t = _torch().arange(5, dtype=_torch().int64, device=c.device)
            c.groups_from_pairs_device(t, t + 1, n_rows=c.n_rows + 5)
        else:
            c.range_search_routed(self.d.q_dev[:3].contiguous(), 0.5, ETA, 0.0)

    def anchor(self, result):
        a64, b64 = self._oracle_pairs()
        assert a64.size >= 200
        if self.which == "pairs":
            a, b, sims = result
            assert np.array_equal(a, a64) and np.array_equal(b, b64)
            assert np.max(np.abs(sims - np.einsum("ij,ij->i", self.d.E[a].astype(np.float64), self.d.E[b].astype(np.float64)))) <= SCORE_TOL
            return
        want = gm.groups(self.d.c.n_rows, a64, b64, keep="dewi", key=self.d.dewi32)
        for got, w in zip(result, want):
            assert np.array_equal(np.asarray(got), np.asarray(w))


class Ivf(Route):
    """``IVFIndex.search_device``: ``_probe_buf``, ``_ivf_ws``, the coarse corpus's workspace."""

    N, D, NLIST, K, NPROBE, B = 20000, 64, 64, 10, 4, 20

    def __init__(self):
        from dewi.ivf import IVFIndex
        X, Q = _clustered(self.N, self.D, 5)
        self.cols = orc.synth_payload_columns(self.N, seed=5)
        self.ivf = IVFIndex(self.D, "cosine", nlist=self.NLIST)
        self.ivf.add_batch_columns([f"doc_{i:07d}" for i in range(self.N)], X, self.cols)
        self.ivf.build()
        self.Q = Q[: self.B]
        self.q_dev = _torch().from_numpy(self.Q).cuda()

    def reset(self):
        self.ivf._probe_buf = self.ivf._ivf_ws = None
        self.ivf._ivf.coarse.drop_cached_workspaces()

    def owners(self):
        return [self.ivf, self.ivf._ivf.coarse]

    def assert_route(self):
        from dewi import ivf as ivf_mod
        assert self.B > 2 * ivf_mod.PROBE_GROUP and self.B % ivf_mod.PROBE_GROUP != 0       # three cell groups, a ragged last one
        assert self.ivf._probe_buf is not None and self.ivf._ivf_ws is not None

    def call(self, guarded):
        return tuple(self.ivf.search_device(self.q_dev, self.K, ETA, 0.0, nprobe=self.NPROBE)), []

    def other(self):
        self.ivf.search_device(self.q_dev[:3].contiguous(), 4, ETA, 0.0, nprobe=2)

    def after(self, result):
        wsg.check_ids(result[0], self.N)

    def anchor(self, result):
        ids, sc = result
        cells = self.ivf.probe(self.Q, self.NPROBE)
        E = self.ivf._embeddings
        dewi32, ent32 = orc.payload_soa(self.cols["dewi"], self.cols["ht_mean"], self.cols["hi_mean"])
        dec = 0
        for j in range(self.B):
            rows = np.flatnonzero(np.isin(self.ivf.cell_of_row, cells[j]))
            pos = np.searchsorted(rows, ids[j])
            assert np.array_equal(rows[np.minimum(pos, rows.size - 1)], ids[j]), "an id outside the probe"
            decisive, msg = compare_query(E[rows], self.Q[j], dewi32[rows], ent32[rows], self.K, ETA, 0.0, "cosine", pos, sc[j])
            assert msg is None, f"query {j}: {msg}"
            dec += int(decisive)
        assert dec >= 0.8 * self.B, f"only {dec}/{self.B} decisive queries"


# ------------------------------------------------------------------------------------------------ the route table
ROW_DIMS_F32 = {768: "scan_rows_f32", 1000: "scan_rows_any<0", 100: "scan_short_rows_any<0", 129: "scan_rows_any<0", 4100: "scan_generic_f32"}
ROW_DIMS_BF16 = {768: "scan_rows_bf16", 1000: "scan_rows_any<1"}
# k -> floor: c = 20 (per-workgroup lists), 80 (per-wave lists), 300 (dense keys), 2050 (the global-memory select)
ROW_KS = {10: 0.8, 40: 0.8, 150: 0.6, 1025: None}
N_MFMA = 65_600                                            # just above the 64 K-row floor of the matrix-core passes


def _row_route(dim, k, kind):
    n = 1500 if dim == 4100 else 3001                      # (k = 1025 at 1500 rows: c = 1500, still beyond the 1024 the LDS select sorts)
    prefix = (ROW_DIMS_F32 if kind == "f32" else ROW_DIMS_BF16)[dim]
    return Search(_synth(n, dim, 5, kind), k, prefix, floor=ROW_KS[k], flags=False, refused=False, other=(3, 7))


def _mfma(dim, b, kind, prefix, space="cosine", shadow_kernel=None, **kw):
    return Search(_synth(N_MFMA, dim, b, kind, space, seed=dim + b, **kw), 10, prefix, floor=0.75, flags=True, refused=False, other=(7, 3),
                  shadow_kernel=shadow_kernel)


def _filtered(short):
    d = _synth(3001, 100, 5)
    mask = np.zeros(3001, dtype=bool)
    mask[np.random.RandomState(1).choice(3001, 15 if short else 900, replace=False)] = True
    return Filtered(d, mask, 10)


def _query_filtered():
    d = _synth(3001, 100, 5)
    rs = np.random.RandomState(2)
    masks = np.zeros((5, 3001), dtype=bool)
    masks[0] = rs.rand(3001) < 0.3
    masks[1, rs.choice(3001, 13, replace=False)] = True    # 10 = k <= |F_1| < c = 20
    masks[3] = rs.rand(3001) < 0.05                        # (masks[2] stays empty)
    masks[4] = True
    return QueryFiltered(d, masks, 10)


def _duplicates(which, shadow):
    key = ("dups", shadow)
    if key not in _corpora:
        n, dim = 3000, 256
        X, Q = _clustered(n, dim, 0, n_queries=8)
        r = np.random.RandomState(1)
        perm = r.permutation(n)
        X[perm[:200]] = _unit(X[perm[200:400]] + 0.01 * r.randn(200, dim))
        X[perm[400:440]] = X[perm[440]]
        _corpora[key] = _Data(X, orc.synth_payload_columns(n, seed=0), Q, "shadow" if shadow else "f32")
    return Duplicates(_corpora[key], which)


def _range(b, shadow):
    key = "range"                                          # one corpus with a shadow; the dense route is use_shadow=False
    if key not in _corpora:
        X, Q = _clustered(3001, 256, 0, n_queries=40)
        _corpora[key] = _Data(X, orc.synth_payload_columns(3001, seed=0), Q, "shadow")
    return Range(_corpora[key], b, 0.3, shadow)


ROUTES = {}
for _dim in ROW_DIMS_F32:
    for _k in ROW_KS:
        ROUTES[f"rows-f32-d{_dim}-k{_k}"] = (lambda dim=_dim, k=_k: _row_route(dim, k, "f32"))
for _dim in ROW_DIMS_BF16:
    for _k in ROW_KS:
        ROUTES[f"rows-bf16-d{_dim}-k{_k}"] = (lambda dim=_dim, k=_k: _row_route(dim, k, "bf16"))
ROUTES.update({
    "mfma-f32-depth-b8": lambda: _mfma(256, 8, "f32", "mfma_scan_f32<false"),
    "mfma-f32-depth-b33-padded-group": lambda: _mfma(256, 33, "f32", "mfma_scan_f32<false"),
    "mfma-f32-partial-chunk-d200": lambda: _mfma(200, 8, "f32", "mfma_scan_f32<false"),
    "mfma-f32-l2-refine-d512-b5": lambda: _mfma(512, 5, "f32", "mfma_scan_f32<false", space="l2"),
    "mfma-bf16-depth-b8": lambda: _mfma(256, 8, "bf16", "mfma_scan_f32<true"),
    "mfma-bf16-256query-b40": lambda: _mfma(256, 40, "bf16", "mfma_scan_bf16_s16"),
    "shadow-depth-b8": lambda: _mfma(256, 8, "shadow", None, shadow_kernel="mfma_scan_f32<true"),
    "shadow-256query-b40": lambda: _mfma(256, 40, "shadow", None, shadow_kernel="mfma_scan_bf16_s16"),
    "shadow-lists-one-query": lambda: Search(_synth(N_MFMA, 256, 8, "shadow", seed=264, single_query=True), 10, None, floor=1.0,
                                             flags=True, refused=False, other=(8, 3), b=1, shadow_kernel="scan_rows_bf16"),
    "refusals-planted-shadow-b8": lambda: Search(_planted("n66000-d256-b8", "shadow"), 10, None, floor=0.75, flags=True, refused=True,
                                                 other=(7, 3), shadow_kernel="mfma_scan_f32<true"),
    "refusals-planted-f32-b32": lambda: Search(_planted("n66000-d256-b32", "f32"), 10, "mfma_scan_f32<false", floor=0.75, flags=True,
                                               refused=True, other=(7, 3)),
    "filtered-shorter-than-the-cut": lambda: _filtered(True),
    "filtered-longer-than-the-cut": lambda: _filtered(False),
    "query-filters-mixed": _query_filtered,
    "shards-merge-lds": lambda: ShardsAndMerge(_synth(3001, 100, 5), [0, 1001, 1003, 3001], 20, 10, 0.8, large=False),
    "shards-merge-global-rank": lambda: ShardsAndMerge(_synth(3001, 100, 5), [0, 1001, 1804, 3001], 700, 350, 0.4, large=True),
    "pipelined-depth3": lambda: Pipelined(_synth(N_MFMA, 256, 8, "f32", seed=264), 10),
    "search-diverse": lambda: Diverse(_synth(3001, 100, 5), 10),
    "range-dense-one-chunk": lambda: _range(8, False),
    "range-dense-two-chunks-ragged": lambda: _range(40, False),
    "range-shadow": lambda: _range(40, True),
    "near-duplicates-dense": lambda: _duplicates("pairs", False),
    "near-duplicates-shadow": lambda: _duplicates("pairs", True),
    "duplicate-groups": lambda: _duplicates("groups", False),
    "groups-from-pairs": lambda: _duplicates("from_pairs", False),
    "ivf-search": Ivf,
})


def _route(name):
    if name not in _routes:
        _routes[name] = ROUTES[name]()
    return _routes[name]


@pytest.mark.parametrize("pattern", wsg.PATTERNS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_results_do_not_depend_on_what_the_workspace_held(route, pattern):
    torch = _torch()
    r = _route(route)
    # 1. caches filled by one warm call
    r.reset()
    warm, _ = r.call(False)
    warm = _host(warm)
    r.assert_route()
    r.after(warm)
    # 2. the oracle, once per route
    if r.base is None:
        r.anchor(warm)
        r.base = warm
    else:
        wsg.assert_bit_equal(warm, r.base, f"{route}: warm call")
    # 3. poisoned, guarded workspaces and outputs
    owners = r.owners()
    try:
        n_guarded = sum(wsg.guard(o) for o in owners)
        assert n_guarded >= 1, "the warm call left no workspace in any cache"
        for i, o in enumerate(owners):
            wsg.poison(o, pattern, seed=16 * i)
        torch.cuda.synchronize()                              # (the fills ran on the current stream; a pipeline has its own)
        got, outs = r.call(True)
        torch.cuda.synchronize()
        got = _host(got)
        wsg.assert_bit_equal(got, r.base, f"{route} after {pattern}")
        r.after(got)
        for o in owners:
            wsg.check(o)
        for out in outs:
            out.check()
        # 4. its own leftovers, another batch size and k, the original call again
        wsg.assert_bit_equal(_host(r.call(False)[0]), r.base, f"{route} on its own leftovers")
        r.other()
        wsg.assert_bit_equal(_host(r.call(False)[0]), r.base, f"{route} after a call of another shape")
        torch.cuda.synchronize()
        for o in owners:
            wsg.check(o, interior=False, in_place=False)
    finally:
        for o in owners:
            wsg.release(o)


# ====================================================================================================== IVF cell lists
@pytest.mark.parametrize("pattern", wsg.PATTERNS)
def test_ivf_lists_built_into_a_poisoned_buffer(pattern):
    """``dewi_ivf_lists_build`` into a guarded buffer under every pattern: bit-equal to the index's own lists (whose every
    segment ``ivf-search`` compares with the assignment through the probe), nothing written outside ``dewi_ivf_lists_bytes``."""
    torch, nat = _torch(), _nat()
    r = _route("ivf-search")
    st, lib = r.ivf._ivf, nat.load_library()
    need = int(lib.dewi_ivf_lists_bytes(r.N, r.D, 0, st.nlist))
    assert need == st.lists.numel()
    offsets, rows, g = r.ivf.cell_lists()                 # the anchor: every (cell, residue) segment against the assignment
    cell = r.ivf.cell_of_row
    for c in range(st.nlist):
        for b in range(g):
            seg = rows[offsets[c * g + b]: offsets[c * g + b + 1]].astype(np.int64)
            assert np.array_equal(seg, np.nonzero((cell == c) & (np.arange(r.N) % g == b))[0]), (c, b)
    buf = wsg.GuardedBuffer(need, st.lists.device, pattern, label="cell lists")
    nat.check(lib.dewi_ivf_lists_build(0, r.N, r.D, st.nlist, nat.ptr(st.assign), nat.ptr(buf.view), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    buf.check()
    bins = st.nlist * st.buckets
    used = 4 * (bins + 1 + r.N + 1)                       # offsets, rows, the error word: what the layout defines
    assert torch.equal(buf.view[:used], st.lists[:used])


# ====================================================================================================== the fit
# dewi_robust_fit_f32 takes the two-launch fast path while robust_fit_fast_supported(n): 2 * per_bucket <= kFitFastCap / kBuckets
# with per_bucket = n * 2 * kDelta / kSample / kBuckets = n * 416 / 4096 / 16 (integer divisions) and kFitFastCap = 2^20,
# kBuckets = 16, i.e. per_bucket <= 32768, n <= 5 162 220.  n = 5 300 000: per_bucket = 33642 -> the histogram path inside the
# monolithic entry point.
FIT_CASES = {"one-workgroup-per-column": (1000, 1000, 3), "two-launch-ld": (300_001, 300_007, 3), "histogram-path": (5_300_000, 5_300_000, 2)}
_fit = {}


def _fit_case(name):
    if name not in _fit:
        n, ld, ns = FIT_CASES[name]
        rs = np.random.RandomState(1)
        host = np.full((ns, ld), 1e9, np.float32)         # padding behind the columns must not be read
        host[:, :n] = rs.gamma(2, 0.5, (ns, n)).astype(np.float32)
        # the anchor: orc.robust_fit's definition (median, median of |x - median|), in the table's own fp32
        want_med = np.array([np.median(host[s, :n]) for s in range(ns)], np.float32)
        want_mad = np.array([np.median(np.abs(host[s, :n] - want_med[s])) for s in range(ns)], np.float32)
        med, mad = orc.robust_fit({f"s{s}": host[s, :n] for s in range(min(ns, 1))})
        assert np.float32(med["s0"]) == want_med[0] and np.float32(mad["s0"]) == want_mad[0]
        _fit[name] = (_torch().from_numpy(host).cuda(), want_med, want_mad)
    return _fit[name]


@pytest.mark.parametrize("pattern", wsg.PATTERNS)
@pytest.mark.parametrize("case", list(FIT_CASES))
def test_robust_fit_through_the_abi_on_a_poisoned_workspace(case, pattern):
    torch, nat = _torch(), _nat()
    lib = nat.load_library()
    n, ld, ns = FIT_CASES[case]
    dev, want_med, want_mad = _fit_case(case)
    need = int(lib.dewi_robust_fit_workspace_bytes(ns))
    assert need > 0
    ws = wsg.GuardedBuffer(need, dev.device, pattern, label="fit workspace")
    med = wsg.GuardedOutput((ns,), torch.float32, dev.device, label="med")
    mad = wsg.GuardedOutput((ns,), torch.float32, dev.device, label="mad")
    for rep in range(2):                                  # poisoned, then on its own leftovers
        nat.check(lib.dewi_robust_fit_f32(nat.ptr(dev), n, ld, ns, nat.ptr(med.mid), nat.ptr(mad.mid), nat.ptr(ws.view), need,
                                          nat.stream_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(med.mid.cpu().numpy(), want_med) and np.array_equal(mad.mid.cpu().numpy(), want_mad), (case, pattern, rep)
        # n = 1000 (at most kSmallN values: one workgroup per column, on chip): all the route leaves in the workspace are the
        # counters its memset zeroed — over a zero fill no byte can differ; the three other patterns show that the workspace
        # was used
        ws.check(interior=not (case == "one-workgroup-per-column" and pattern == "zeros"))
        med.check()
        mad.check()


@pytest.mark.parametrize("pattern", wsg.PATTERNS)
def test_fit_steps_on_a_poisoned_workspace(pattern):
    """``HipFitSteps``: begin, then hist / pick per pass and finish per phase (``ShardedRobustFit`` on one rank drives them)."""
    from dewi.sharded import HipFitSteps, ShardedRobustFit
    torch = _torch()
    dev, want_med, want_mad = _fit_case("two-launch-ld")
    n = FIT_CASES["two-launch-ld"][0]
    steps = HipFitSteps(dev[:, :n])
    ws = wsg.GuardedBuffer(steps.ws_bytes, dev.device, pattern, label="fit-steps workspace")
    steps.ws = ws.view
    for rep in range(2):
        med, mad = ShardedRobustFit(steps, n).fit()
        torch.cuda.synchronize()
        assert np.array_equal(np.asarray(med, np.float32), want_med) and np.array_equal(np.asarray(mad, np.float32), want_mad), rep
        ws.check()

"""Host side of the search entry points (no GPU): the one argument check, the one cut rule and the one workspace cache of
``dewi._engine``, each driven as a plain function of shapes and values."""
import threading
import types

import pytest


def _eng():
    from dewi import _engine
    return _engine


# ---------------------------------------------------------------------------------------------------------- the cut rule
# (k, candidates, rows) -> the cut each call site derived before it had one rule to call; n = 1000 corpus rows, |A| = 15 / 7
CUT_SITES = {
    # DeviceCorpus.search_device: max(min(2k, N) or min(candidates, N), 1), the workspace's and the refusal flags' cut
    "search_device": (lambda k, cand: (k, cand, 1000),
                      [((10, None), 20), ((600, None), 1000), ((10, 10), 10), ((10, 5000), 1000), ((10, 0), 1), ((10, -3), 1)]),
    # _search_filtered (k > 0, |A| > 0): min(2k, |A|) or min(max(candidates, 1), |A|)
    "search_filtered": (lambda k, cand: (k, cand, 15),
                        [((5, None), 10), ((10, None), 15), ((5, 7), 7), ((5, 40), 15), ((5, 0), 1), ((1, None), 2)]),
    "search_filtered_short": (lambda k, cand: (k, cand, 7), [((5, None), 7), ((5, 5), 5), ((7, 30), 7)]),
    # _search_query_filtered (k > 0): 2k or max(candidates, 1), no cap (shorter lists leave the shared pass)
    "search_query_filtered": (lambda k, cand: (k, cand, None), [((10, None), 20), ((10, 30), 30), ((10, 0), 1), ((1, None), 2)]),
    # IVFIndex.search_device (k > 0, candidates >= k): 2k or candidates, no cap
    "ivf_search_device": (lambda k, cand: (k, cand, None), [((10, None), 20), ((10, 10), 10), ((3, 4000), 4000)]),
    # scan_kernel_name: the same as search_device (k may be 0 there: the floor)
    "scan_kernel_name": (lambda k, cand: (k, cand, 1000), [((10, None), 20), ((0, None), 1), ((700, None), 1000), ((10, 64), 64)]),
    # PipelinedSearcher's workspace: max(1, min(c, N)) of its own c (n_candidates, or min(2k, N))
    "pipelined_workspace": (lambda k, c: (k, c, 1000), [((10, 20), 20), ((10, 4000), 1000), ((10, 0), 1), ((0, 0), 1)]),
}


@pytest.mark.parametrize("site", sorted(CUT_SITES))
def test_cut_rule_reproduces_every_call_site(site):
    args_of, table = CUT_SITES[site]
    for (k, cand), want in table:
        assert _eng().cut_size(*args_of(k, cand)) == want, (site, k, cand)


def test_cut_rule_takes_numpy_integers():
    import numpy as np
    assert _eng().cut_size(np.int64(4), None, np.int64(5)) == 5
    assert _eng().cut_size(4, np.int32(6)) == 6


# ---------------------------------------------------------------------------------------------------------- the argument check
def test_argument_check_messages_and_order():
    check = _eng().check_search_args
    assert check((3, 8), 8, 10, None, "ip") == (3, 10)
    assert check((1, 8), 8, "4", 4, "one_minus_dist") == (1, 4)               # k is made an int, as before
    assert check((2, 8), 8, 0, None, "ip") == (2, 0)                          # k <= 0 is not its business
    with pytest.raises(ValueError, match=r"^Expected query shape \(8,\), got \(7,\)$"):
        check((3, 7), 8, 10, None, "ip")
    with pytest.raises(ValueError, match=r"^unknown similarity 'cosine'$"):
        check((3, 8), 8, 10, None, "cosine")
    with pytest.raises(ValueError, match=r"^similarity transforms belong to the ANN re-rank rule: pass candidates=k as well$"):
        check((3, 8), 8, 10, None, "inv_one_plus_dist")
    # one order for every caller: width, similarity, the transform rule
    with pytest.raises(ValueError, match="Expected query shape"):
        check((3, 7), 8, 10, None, "cosine")
    with pytest.raises(ValueError, match="unknown similarity"):
        check((3, 8), 8, 0, None, "nope")


def test_unfiltered_search_checks_similarity_before_k():
    """k <= 0 with an unknown similarity raises on the unfiltered path as on the other three (it used to return [B, 0])."""
    import torch
    eng = _eng()
    c = types.SimpleNamespace(dim=4, n_rows=10, device=torch.device("cpu"))
    q = torch.zeros((3, 4))
    with pytest.raises(ValueError, match="unknown similarity 'nope'"):
        eng.DeviceCorpus.search_device(c, q, 0, 0.3, 0.0, similarity="nope")
    with pytest.raises(ValueError, match="pass candidates=k as well"):
        eng.DeviceCorpus.search_device(c, q, -1, 0.3, 0.0, similarity="one_minus_dist")
    ids, sc = eng.DeviceCorpus.search_device(c, q, 0, 0.3, 0.0)
    assert ids.shape == (3, 0) and ids.dtype == torch.int64 and sc.shape == (3, 0) and sc.dtype == torch.float32


def test_empty_result_and_default_outputs():
    import torch
    eng = _eng()
    dev = torch.device("cpu")
    ids, sc = eng.default_outputs(2, 5, dev)
    assert ids.shape == (2, 5) and ids.dtype == torch.int64 and sc.shape == (2, 5) and sc.dtype == torch.float32
    mine = torch.zeros((2, 5), dtype=torch.int64)
    ids2, sc2 = eng.default_outputs(2, 5, dev, mine, None)
    assert ids2 is mine and sc2.shape == (2, 5)
    ids3, sc3 = eng.default_outputs(2, 5, dev, mine, sc)
    assert ids3 is mine and sc3 is sc


# ---------------------------------------------------------------------------------------------------------- the host split
class _SplitCorpus:
    """What ``_split_query_lists`` touches of a corpus: the device and the two filter factories, which record their masks."""

    def __init__(self):
        import torch
        self.device = torch.device("cpu")
        self.made_subsets, self.made_singles = [], []

    def make_query_filters(self, masks):
        self.made_subsets.append(masks.clone())
        return ("subset", len(self.made_subsets))

    def make_filter(self, mask):
        self.made_singles.append(mask.clone())
        return ("single", len(self.made_singles))


def _split(counts, c, k=2, corpus=None, qf=None):
    """Run the split over lists of the given lengths with callables that record their arguments and write a mark per row:
    shared passes write 100 + (row within the pass), single lists 200."""
    import torch
    eng = _eng()
    b = len(counts)
    corpus = corpus or _SplitCorpus()
    masks = (torch.arange(b * 6).reshape(b, 6) % 3 == 0).to(torch.uint8)
    qf = qf or types.SimpleNamespace(n_allowed=list(counts), masks=masks, _subsets={}, _singles={})
    qf.n_allowed = list(counts)
    q = torch.arange(b * 4, dtype=torch.float32).reshape(b, 4)
    ids = torch.full((b, k), 7, dtype=torch.int64)
    sc = torch.zeros((b, k))
    calls = []

    def run_shared(sub, q_sub, o_ids, o_sc):
        calls.append(("shared", sub, q_sub.clone(), o_ids is ids, tuple(o_ids.shape)))
        assert q_sub.is_contiguous()
        o_ids.copy_(100 + torch.arange(o_ids.shape[0]).reshape(-1, 1).expand_as(o_ids))
        o_sc.fill_(1.0)

    def run_single(f, q_1, o_ids, o_sc):
        calls.append(("single", f, q_1.clone(), tuple(o_ids.shape)))
        o_ids.fill_(200)
        o_sc.fill_(2.0)

    got = eng.DeviceCorpus._split_query_lists(corpus, qf, q, k, c, ids, sc, run_shared, run_single)
    assert got[0] is ids and got[1] is sc
    return corpus, qf, q, ids, sc, calls


def test_split_all_lists_long():
    corpus, qf, q, ids, sc, calls = _split([9, 5, 5], c=5)
    assert len(calls) == 1 and calls[0][0] == "shared" and calls[0][1] is qf           # the filters themselves, the caller's outputs
    assert calls[0][3] is True and (calls[0][2] == q).all()
    assert corpus.made_subsets == [] and corpus.made_singles == [] and qf._subsets == {} and qf._singles == {}
    assert ids.tolist() == [[100, 100], [101, 101], [102, 102]] and (sc == 1.0).all()


def test_split_some_short_some_empty():
    import torch
    corpus, qf, q, ids, sc, calls = _split([9, 3, 0, 5, 1], c=5)
    kinds = [c[0] for c in calls]
    assert kinds == ["shared", "single", "single"]                                      # the shared pass first, then in query order
    shared = calls[0]
    assert shared[1] == ("subset", 1) and shared[3] is False and shared[4] == (2, 2)    # outputs of its own, copied back
    assert (shared[2] == q[[0, 3]]).all()
    assert list(qf._subsets) == [(0, 3)] and (corpus.made_subsets[0] == qf.masks[[0, 3]].view(torch.bool)).all()
    assert corpus.made_subsets[0].dtype == torch.bool
    assert [c[1] for c in calls[1:]] == [("single", 1), ("single", 2)] and sorted(qf._singles) == [1, 4]
    assert (calls[1][2] == q[1:2]).all() and (calls[2][2] == q[4:5]).all() and calls[1][3] == (1, 2)
    assert (corpus.made_singles[0] == qf.masks[1].view(torch.bool)).all()
    assert ids.tolist() == [[100, 100], [200, 200], [-1, -1], [101, 101], [200, 200]]
    assert sc[[0, 3]].eq(1.0).all() and sc[[1, 4]].eq(2.0).all() and torch.isnan(sc[2]).all()
    # the same batch again: both caches hit, nothing is prepared twice
    _split([9, 3, 0, 5, 1], c=5, corpus=corpus, qf=qf)
    assert len(corpus.made_subsets) == 1 and len(corpus.made_singles) == 2


def test_split_all_short_or_empty():
    import torch
    corpus, qf, q, ids, sc, calls = _split([2, 0, 4], c=5)
    assert [c[0] for c in calls] == ["single", "single"] and corpus.made_subsets == [] and sorted(qf._singles) == [0, 2]
    assert ids.tolist() == [[200, 200], [-1, -1], [200, 200]] and torch.isnan(sc[1]).all()
    corpus, qf, q, ids, sc, calls = _split([0, 0], c=5)
    assert calls == [] and ids.tolist() == [[-1, -1], [-1, -1]] and torch.isnan(sc).all()


def test_split_subset_cache_is_cleared_beyond_eight_entries():
    corpus = _SplitCorpus()
    qf = None
    for i in range(9):                               # nine distinct subsets of a batch of ten: {i, 9}
        counts = [0] * 10
        counts[i] = counts[9] = 5
        corpus, qf, *_ = _split(counts, c=5, corpus=corpus, qf=qf)
    assert len(qf._subsets) == 9                     # the rule as it is: cleared before a preparation that finds MORE than 8
    counts = [5, 5] + [0] * 8
    _split(counts, c=5, corpus=corpus, qf=qf)
    assert list(qf._subsets) == [(0, 1)] and len(corpus.made_subsets) == 10
    assert qf._singles == {}


# ---------------------------------------------------------------------------------------------------------- the blocking twins
def test_blocking_id_rules(monkeypatch):
    import contextlib
    import numpy as np
    import torch
    eng = _eng()
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    staged = []

    def corpus(id_offset):
        def stage(queries):
            staged.append(queries)
            return torch.as_tensor(queries)
        return types.SimpleNamespace(_lock=threading.RLock(), device=torch.device("cpu"), id_offset=id_offset, stage_queries=stage)

    def search(q, k, tag):
        assert tag == "tag" and k == 3 and q.shape == (2, 4)
        return torch.tensor([[4, -1, 0], [2, 1, -1]]), torch.tensor([[0.5, float("nan"), 0.25], [1.0, 0.5, float("nan")]])

    q = np.zeros((2, 4), np.float32)
    blocking = eng.DeviceCorpus._blocking
    ids, sc = blocking(corpus(1000), search, q, 3, "tag")
    assert ids.tolist() == [[1004, 999, 1000], [1002, 1001, 999]] and ids.dtype == np.int64      # "offset": every id
    assert sc.dtype == np.float32 and sc[0, 0] == 0.5 and np.isnan(sc[0, 1])
    ids, _ = blocking(corpus(1000), search, q, 3, "tag", ids="offset_valid")
    assert ids.tolist() == [[1004, -1, 1000], [1002, 1001, -1]]                                  # -1 stays -1
    ids, _ = blocking(corpus(1000), search, q, 3, "tag", ids="global")
    assert ids.tolist() == [[4, -1, 0], [2, 1, -1]]                                              # as the records carried them
    for rule in ("offset", "offset_valid", "global"):
        ids, _ = blocking(corpus(0), search, q, 3, "tag", ids=rule)
        assert ids.tolist() == [[4, -1, 0], [2, 1, -1]]
    assert len(staged) == 6 and all(s is q for s in staged)


# ---------------------------------------------------------------------------------------------------------- the workspace cache
class _Sizes:
    """A fake size function: counts its calls, answers what it is told to."""
    __name__ = "fake_workspace_bytes"

    def __init__(self, need):
        self.need, self.calls = need, []

    def __call__(self, *args):
        self.calls.append(args)
        return self.need


def _corpus():
    import torch
    return types.SimpleNamespace(_ws={}, device=torch.device("cpu"))


@pytest.fixture
def tuning(monkeypatch):
    """``_engine.tuning`` with a library stub behind it (the real call needs a device): what it does to the epochs is real."""
    eng = _eng()
    stub = types.SimpleNamespace(dewi_tuning_set=lambda *a: 0)
    monkeypatch.setattr(eng.nat, "load_library", lambda *a, **kw: stub)
    return eng.tuning


def test_workspace_cache_hit_epoch_growth(tuning):
    cached = _eng().DeviceCorpus._cached_workspace
    c, size = _corpus(), _Sizes(100)
    ws = cached(c, ("filtered", 2, 8192, 20), size, 8192, 256, 2, 20)
    assert ws.numel() == 100 and str(ws.dtype) == "torch.uint8" and size.calls == [(8192, 256, 2, 20)]
    assert cached(c, ("filtered", 2, 8192, 20), size, 8192, 256, 2, 20) is ws and len(size.calls) == 1     # a hit: no size call
    tuning(scan_blocks=8)
    size.need = 60                                    # a smaller plan: one size call, the tensor stays
    assert cached(c, ("filtered", 2, 8192, 20), size, 8192, 256, 2, 20) is ws and len(size.calls) == 2
    assert cached(c, ("filtered", 2, 8192, 20), size, 8192, 256, 2, 20) is ws and len(size.calls) == 2
    tuning()
    size.need = 640                                   # a larger plan (the stale-workspace defect): one size call, a new tensor
    grown = cached(c, ("filtered", 2, 8192, 20), size, 8192, 256, 2, 20)
    assert grown is not ws and grown.numel() == 640 and len(size.calls) == 3 and len(c._ws) == 1
    assert cached(c, ("filtered", 2, 8192, 20), size, 8192, 256, 2, 20) is grown and len(size.calls) == 3
    other = cached(c, (2, 20), size, 1)               # another key: its own tensor
    assert other is not grown and len(c._ws) == 2


def test_workspace_cache_size_zero_raises():
    from dewi import _native as nat
    cached = _eng().DeviceCorpus._cached_workspace
    c = _corpus()
    with pytest.raises(nat.NativeLibraryError, match=r"^fake_workspace_bytes returned 0: "):
        cached(c, (1, 20), _Sizes(0), 1, 20)
    assert c._ws == {}


def test_workspace_cache_eviction_beyond_eight_entries():
    cached = _eng().DeviceCorpus._cached_workspace
    c, size = _corpus(), _Sizes(16)
    first = [cached(c, (b, 20), size, b) for b in range(1, 10)]
    assert len(c._ws) == 9                            # the rule as it was: dropped before an allocation that finds MORE than 8
    assert cached(c, (1, 20), size, 1) is first[0] and len(size.calls) == 9
    cached(c, (10, 20), size, 10)
    assert list(c._ws) == [(10, 20)]
    assert cached(c, (1, 20), size, 1) is not first[0] and len(c._ws) == 2


def test_workspace_cache_accessors(tuning):
    """``cached_workspaces`` / ``replace_cached_workspace`` / ``drop_cached_workspaces`` (what tests/wsguard.py swaps the
    tensors through): a copy of the table, the tuning epoch of the entry kept, a smaller tensor refused, the cache emptied."""
    import torch
    dc = _eng().DeviceCorpus
    c, size = _corpus(), _Sizes(100)
    tuning(scan_blocks=8)                             # an epoch other than the defaults' 0
    ws = dc._cached_workspace(c, (2, 20), size, 2)
    other = dc._cached_workspace(c, ("range", 3, 9), size, 3)
    epoch = c._ws[(2, 20)][1]
    assert epoch != 0
    table = dc.cached_workspaces(c)
    assert list(table) == [(2, 20), ("range", 3, 9)] and table[(2, 20)] is ws and table[("range", 3, 9)] is other
    table.clear()                                     # a copy: the cache itself is untouched
    assert len(c._ws) == 2
    big = torch.zeros(4096 + 100 + 4096, dtype=torch.uint8)
    view = big[4096: 4096 + 100]
    dc.replace_cached_workspace(c, (2, 20), view)
    assert c._ws[(2, 20)][0] is view and c._ws[(2, 20)][1] == epoch
    assert dc._cached_workspace(c, (2, 20), size, 2) is view and len(size.calls) == 2          # a hit: no size call, the view stays
    assert c._ws[("range", 3, 9)][0] is other
    with pytest.raises(ValueError, match=r"99 bytes replace 100"):
        dc.replace_cached_workspace(c, (2, 20), big[:99])
    assert c._ws[(2, 20)][0] is view
    with pytest.raises(KeyError):
        dc.replace_cached_workspace(c, (7, 7), view)
    dc.drop_cached_workspaces(c)
    assert c._ws == {} and dc.cached_workspaces(c) == {}
    assert dc._cached_workspace(c, (2, 20), size, 2) is not view and len(size.calls) == 3      # allocated afresh


def test_workspace_cache_epochs_belong_to_threads(tuning):
    """A tuning() in another thread leaves this thread's entry valid, and the other way round; a fresh thread — whatever
    ident it gets — starts from the defaults' epoch, not from a dead thread's."""
    eng = _eng()
    cached = eng.DeviceCorpus._cached_workspace
    c, size = _corpus(), _Sizes(100)
    key = (1, 20)

    def in_thread(fn):
        out = []
        t = threading.Thread(target=lambda: out.append(fn()))
        t.start()
        t.join()
        return out[0]

    tuning(scan_blocks=8)                             # this thread: an epoch of its own
    mine = getattr(eng._thread_tuning, "epoch")
    ws = cached(c, key, size, 1, 20)
    assert len(size.calls) == 1
    in_thread(lambda: tuning(scan_blocks=4))          # another thread tunes: nothing changes here
    assert getattr(eng._thread_tuning, "epoch") == mine
    assert cached(c, key, size, 1, 20) is ws and len(size.calls) == 1
    # the other way round: an entry a worker sized under its tuning survives a tuning() of this thread, as seen by the worker
    c2, size2 = _corpus(), _Sizes(100)
    started, tuned, done = threading.Event(), threading.Event(), threading.Event()
    seen = []

    def worker():
        tuning(rows_per_iter=2)
        seen.append(cached(c2, key, size2, 1, 20))
        started.set()
        tuned.wait(10)
        seen.append(cached(c2, key, size2, 1, 20))
        done.set()
    t = threading.Thread(target=worker)
    t.start()
    assert started.wait(10)
    tuning(scan_blocks=16)
    tuned.set()
    assert done.wait(10)
    t.join()
    assert seen[0] is seen[1] and len(size2.calls) == 1
    # fresh threads have the defaults' epoch 0 and never a tuned thread's
    assert in_thread(lambda: getattr(eng._thread_tuning, "epoch", 0)) == 0
    epochs = {in_thread(lambda: (tuning(), getattr(eng._thread_tuning, "epoch"))[1]) for _ in range(4)}
    assert len(epochs) == 4 and mine not in epochs and 0 not in epochs
    # ... so an entry sized by a tuned thread is asked for again by a fresh one
    assert in_thread(lambda: cached(c, key, size, 1, 20)) is ws and len(size.calls) == 2

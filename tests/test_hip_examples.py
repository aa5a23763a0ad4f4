"""GPU tests of the search by examples (``dewi_knn_candidates_examples``; ``ExactIndex.search_by_examples``).

Contract (include/dewi_hip.h, restated in ``examples_model``): every row gets ONE score from its similarities to the P + N
examples, each similarity bit for bit what the one-query search reports; the c best offered rows leave as candidate records.
So the tests take each example's per-row similarities from the library itself (``range_search`` with a threshold nothing
fails: a row that is missing has a NaN similarity), feed them to the model and require IDENTICAL records — id, sim bits,
payload pair.  Outputs sit between guard rows, the workspace between guard bytes and arrives full of garbage.
"""
import numpy as np
import pytest
import torch

import corpora
import dewi_oracle as orc
import examples_model as xm
import parity
import wsguard

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = [132, 256, 388, 768, 1000, 1536, 2052, 4096]     # 1, 1, 2, 3, 4, 6, 9 (held as 10) and 16 units per lane; 256 / 768 / 1536
                                                        # are widths of the tuned one-query kernel; 4 examples per pass up to
                                                        # 1536, 2 at 2052 and 4096
REQUESTS = [(1, 0), (1, 1), (3, 1), (4, 0), (2, 3), (4, 4), (8, 8), (5, 0)]   # (5, 0) runs with match="all"
CUTS = [1, 64, 65, 256, 257, 2048]                      # one sorted list per workgroup | one list per wave | dense keys
WEIGHTS = [0.0, 0.5, 1.0, 2.0]


def _eng():
    from dewi import _engine
    return _engine


def _nat():
    from dewi import _native
    return _native


def rows_in_flight(dim):
    """csrc/scan_any.hpp ``any_level`` / ``any_rows`` for a row of dim / 4 units: the rows a wave loads before it reduces."""
    units = dim // 4
    u = next(v for v in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16) if v >= (units + 63) // 64)
    if u == 1:
        return 12 if units <= 40 else 8
    if u == 2:
        return 6 if units <= 72 else (4 if units <= 92 else 3)
    if u == 3:
        return 2
    if u == 4:
        return 2 if units <= 224 else 1
    return 1


def main_rows(dim):
    """A row count at which a pass runs 4 workgroups (32 waves), every wave its main loop three or four times (127 whole
    groups of R rows) and then R - 1 waves the tail loop (R - 1 rows are left: not a multiple of the R rows in flight).
    dim 132: 1535 rows, 256: 1023, 388: 383, 768: 255."""
    r = rows_in_flight(dim)
    assert r > 1
    return 127 * r + r - 1


def row_counts(dim):
    return [1, 63, main_rows(dim)] if dim <= 768 else [2053]


DUP_FIRST, DUP_LAST, ZERO_ROW = 4, 8, 11                 # rows 5 .. 8 repeat row 4 (ties: the lower row first); row 11 is zero


def _raw(kind, n, dim, seed):
    if kind == "emb":
        m = max(n, 256)
        X = corpora.embedding_like(m, dim, seed)[0][np.linspace(0, m - 1, n).astype(np.int64)].copy()
    else:
        X = orc.synth_corpus(n, dim, seed)
    if n >= 32:
        X[DUP_FIRST + 1: DUP_LAST + 1] = X[DUP_FIRST]
        X[ZERO_ROW] = 0.0                                 # stored as a NaN row: every similarity to it is NaN
    return X


def _corpus(kind, n, dim, seed, id_offset=0):
    raw = _raw(kind, n, dim, seed)
    cols = orc.synth_payload_columns(n, seed=seed)
    c = _eng().DeviceCorpus.from_host(raw, cols["dewi"], cols["ht_mean"], cols["hi_mean"], "cosine", id_offset=id_offset)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    return c, raw, dewi32, ent32


def _example_pool(kind, raw, seed):
    """16 raw examples: [0:8] the positives' pool, [8:16] the negatives'.  Embedding-like: noisy copies of corpus rows (every
    cosine positive).  Gaussian: free directions and a few noisy copies, scaled (examples arrive un-normalised)."""
    rs = np.random.RandomState(seed)
    n, dim = raw.shape
    live = np.array([i for i in range(n) if n < 32 or i != ZERO_ROW])
    base = raw[rs.choice(live, 16, replace=n < 64)].astype(np.float64)
    if kind == "emb":
        X = base + 0.1 / np.sqrt(dim) * rs.randn(16, dim)
    else:
        X = rs.randn(16, dim)
        X[[1, 9]] = base[[1, 9]] * np.sqrt(dim) + 0.5 * rs.randn(2, dim)
    return (X * rs.uniform(0.5, 3.0, (16, 1))).astype(F)


def _request(pool, n_pos, n_neg):
    return np.concatenate([pool[:n_pos], pool[8: 8 + n_neg]])


def _sims(c, X, filt=None):
    """The library's own similarities: fp32 [E, n_rows], NaN where the range search did not return the row."""
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=F)).to(c.device)
    lims, rows, sims, _ = c.range_search_device(x, -2.0, 0.0, 0.0, filter=filt, sort=False)
    lims, rows, sims = lims.cpu().numpy(), rows.cpu().numpy() - c.id_offset, sims.cpu().numpy()
    S = np.full((X.shape[0], c.n_rows), np.nan, F)
    for j in range(X.shape[0]):
        S[j, rows[lims[j]: lims[j + 1]]] = sims[lims[j]: lims[j + 1]]
    return S


_PATTERNS = wsguard.PATTERNS
_calls = [0]


def _call(c, X, n_pos, cut, match="any", rule="penalty", w=1.0, exclude=None, filt=None, expect=0, writes=None, override=None):
    """``dewi_knn_candidates_examples`` straight through the C ABI: records [cut] on the host.  The workspace is exactly
    ``dewi_knn_examples_workspace_bytes`` between guards, prefilled with the next pattern; the output lies between guard rows.
    ``expect``: the status the call must return; ``writes=False`` (the default for a failure): it must write nothing."""
    writes = expect == 0 if writes is None else writes
    nat, lib = _nat(), c._lib
    _calls[0] += 1
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=F)).to(c.device)
    n_scan = c.n_rows if filt is None else filt.n_allowed
    need = int(lib.dewi_knn_examples_workspace_bytes(n_scan, c.dim, max(1, min(16, X.shape[0])), max(1, min(cut, 2048))))
    need = need or 4096
    ws = wsguard.GuardedBuffer(need, c.device, _PATTERNS[_calls[0] % len(_PATTERNS)], "examples workspace", seed=_calls[0])
    out = wsguard.GuardedOutput((max(cut, 1), 4), torch.int32, c.device, label="example records")
    ex = None if exclude is None else torch.tensor(list(exclude), dtype=torch.int64, device=c.device)
    a = dict(d_E=nat.ptr(c.emb), n_rows=c.n_rows, dim=c.dim, d_x=nat.ptr(x), n_pos=n_pos, n_neg=X.shape[0] - n_pos,
             match=nat.EXAMPLES_MATCH_CODES.get(match, match), rule=nat.EXAMPLES_RULE_CODES.get(rule, rule), w=float(w),
             d_ex=nat.ptr(ex) if ex is not None and ex.numel() else None, n_ex=0 if ex is None else int(ex.numel()),
             d_filter=nat.ptr(filt.buf) if filt is not None else None, n_allowed=n_scan if filt is not None else 0,
             d_dewi=nat.ptr(c.dewi32), d_ent=nat.ptr(c.ent32), cut=cut, id_offset=c.id_offset, d_out=nat.ptr(out.mid),
             d_ws=nat.ptr(ws.view), ws_bytes=need)
    a.update(override or {})
    rc = lib.dewi_knn_candidates_examples(a["d_E"], a["n_rows"], a["dim"], a["d_x"], a["n_pos"], a["n_neg"], a["match"], a["rule"],
                                          a["w"], a["d_ex"], a["n_ex"], a["d_filter"], a["n_allowed"], a["d_dewi"], a["d_ent"],
                                          a["cut"], a["id_offset"], a["d_out"], a["d_ws"], a["ws_bytes"], nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect, nat.last_error())
    if not writes:
        ws.check(interior=False)
        assert torch.equal(ws.view, ws._slot.fill[wsguard.G: wsguard.G + need]), "a refused call wrote into the workspace"
        assert bool((out.full.view(torch.uint8) == wsguard.SENTINEL).all()), "a refused call wrote into the output"
        return None
    ws.check(interior=n_scan > 1)      # (one row whose score is NaN: its key is all ones, which is also one of the fills)
    out.check()
    return _eng().records_to_numpy(out.mid)


def _same_records(got, want, what):
    assert np.array_equal(got["id"], want["id"]), (what, got["id"][:12].tolist(), want["id"][:12].tolist())
    for f in ("sim", "dewi", "ent"):
        g, w = got[f].view(np.uint32), want[f].view(np.uint32)
        assert np.array_equal(g, w), (what, f, int(np.flatnonzero(g != w)[0]))


def _check(c, S, X_idx, X, n_pos, cut, match, rule, w, dewi32, ent32, what, exclude=None, filt=None, rows=None):
    score = xm.combine(S[X_idx], n_pos, match, rule, w)
    if rows is not None:
        score = score[rows]
    want = xm.records(score, rows, dewi32, ent32, cut, exclude or (), c.id_offset)
    got = _call(c, X, n_pos, cut, match, rule, w, exclude=exclude, filt=filt)
    _same_records(got, want, what)
    return score


# ------------------------------------------------------------------------------------------------------ 1. bit parity
@pytest.mark.parametrize("kind", ["emb", "gauss"])
@pytest.mark.parametrize("dim", DIMS)
def test_records_equal_the_model(dim, kind):
    seen = dict(clamp=False, pays=False, wins=False, loses=False)
    for n in row_counts(dim):
        c, raw, dewi32, ent32 = _corpus(kind, n, dim, seed=dim + n)
        pool = _example_pool(kind, raw, seed=dim + n + 1)
        S = _sims(c, pool)                                                    # computed once, shared by every request below
        ok = ~np.isnan(S)
        if n >= 32:
            assert np.isnan(S[:, ZERO_ROW]).all() and ok[:, :ZERO_ROW].all()     # the zero row: NaN; nothing else
            assert np.array_equal(S[:, DUP_FIRST].view(np.uint32), S[:, DUP_LAST].view(np.uint32))
        if kind == "emb":
            assert (S[ok] > 0).all()                                          # all cosines positive: n > 0 everywhere
        step = 0
        for n_pos, n_neg in REQUESTS:
            idx = list(range(n_pos)) + list(range(8, 8 + n_neg))
            X = pool[idx]
            match = "all" if (n_pos, n_neg) == (5, 0) else ("any", "all")[step % 2]
            rule = ("penalty", "best_score")[(step // 2) % 2]
            w = WEIGHTS[step % 4]
            cut = CUTS[step % len(CUTS)]
            step += 1
            score = _check(c, S, idx, X, n_pos, cut, match, rule, w, dewi32, ent32, (dim, kind, n, n_pos, n_neg, cut))
            if n >= 32:
                assert np.isnan(score[ZERO_ROW]) and score[DUP_FIRST].view(np.uint32) == score[DUP_LAST].view(np.uint32)
            if n_neg:
                nn = np.fmax.reduce(S[idx][n_pos:], axis=0)
                pp = (np.fmin if match == "all" else np.fmax).reduce(S[idx][:n_pos], axis=0)
                seen["clamp"] |= bool((nn[ok[0]] <= 0).any())
                seen["pays"] |= bool((nn[ok[0]] > 0).any())
                if rule == "best_score":
                    seen["wins"] |= bool((pp[ok[0]] > nn[ok[0]]).any())
                    seen["loses"] |= bool((pp[ok[0]] <= nn[ok[0]]).any())
        # every slot class on one chained request, both rules
        idx = [0, 1, 2, 8, 9]
        for i, cut in enumerate(CUTS):
            _check(c, S, idx, pool[idx], 3, cut, "any", ("penalty", "best_score")[i % 2], 0.5, dewi32, ent32, (dim, kind, n, "cut", cut))
        # edge-value examples: one NaN example (every score NaN: the cut is the lowest rows), one zero example (similarity 0)
        bad = pool.copy()
        bad[8, 3] = np.nan
        bad[1] = 0.0
        Sb = _sims(c, bad[[0, 1, 8]])
        assert np.isnan(Sb[2]).all() and (Sb[1][~np.isnan(Sb[1])] == 0).all()
        _check(c, Sb, [0, 1, 2], bad[[0, 1, 8]], 2, 65, "any", "penalty", 1.0, dewi32, ent32, (dim, kind, n, "nan example"))
        _check(c, Sb, [0, 1], bad[[0, 1]], 2, 20, "all", "penalty", 1.0, dewi32, ent32, (dim, kind, n, "zero example"))
        _check(c, Sb, [0, 1], bad[[0, 1]], 1, 20, "any", "best_score", 1.0, dewi32, ent32, (dim, kind, n, "zero negative"))
    if kind == "gauss":
        assert all(seen.values()), seen        # the penalty's clamp and best_score's else-branch really ran
    else:
        assert seen["pays"] and not seen["clamp"], seen


@pytest.mark.parametrize("dim", [388, 768])
def test_rules_crossed(dim):
    """Every request x match x rule x weight x cut on one corpus (127 groups and a tail, four workgroups)."""
    n = main_rows(dim)
    c, raw, dewi32, ent32 = _corpus("gauss", n, dim, seed=dim)
    pool = _example_pool("gauss", raw, seed=dim + 1)
    S = _sims(c, pool)
    for n_pos, n_neg in REQUESTS:
        idx = list(range(n_pos)) + list(range(8, 8 + n_neg))
        for match in ("any", "all"):
            for rule in ("penalty", "best_score") if n_neg else ("penalty",):
                for w in WEIGHTS if (n_neg and rule == "penalty") else (1.0,):
                    for cut in CUTS:
                        _check(c, S, idx, pool[idx], n_pos, cut, match, rule, w, dewi32, ent32, (n_pos, n_neg, match, rule, w, cut))


# ------------------------------------------------------------------------------------------------------ 2. pass split
@pytest.mark.parametrize("dim", [768, 2052])
def test_pass_split_changes_no_bit(dim):
    n = 2053
    c, raw, dewi32, ent32 = _corpus("gauss", n, dim, seed=dim + 5)
    pool = _example_pool("gauss", raw, seed=dim + 6)
    f = c.make_filter(np.random.RandomState(dim).rand(n) < 0.4)
    lib = c._lib
    for n_pos, n_neg in [(8, 8), (3, 1), (2, 3), (4, 4), (5, 0)]:
        X = _request(pool, n_pos, n_neg)
        for cut, rule, filt in ((64, "penalty", None), (257, "best_score", None), (100, "penalty", f)):
            match = "all" if n_neg == 0 else "any"
            base = _call(c, X, n_pos, cut, match, rule, 0.5, exclude=[3, 70], filt=filt)
            for per_pass in (1, 2):
                assert lib.dewi_examples_tuning_set(per_pass) == 0
                try:
                    got = _call(c, X, n_pos, cut, match, rule, 0.5, exclude=[3, 70], filt=filt)
                finally:
                    assert lib.dewi_examples_tuning_set(0) == 0
                _same_records(got, base, (dim, n_pos, n_neg, cut, per_pass))


# ------------------------------------------------------------------------------------------------------ 3. one example
def _index(n, dim, seed, cls=None, **kw):
    from dewi.backends import ExactIndex
    from dewi.types import payloads_from_columns
    raw = orc.synth_corpus(n, dim, seed=seed)
    cols = orc.synth_payload_columns(n, seed=seed)
    idx = (cls or ExactIndex)(dim, "cosine", **kw)
    idx.add_batch([f"d{i}" for i in range(n)], raw, payloads_from_columns(cols))
    idx.build()
    return idx, raw, cols


def _pairs(res):
    return [(d, F(s).view(np.uint32)) for d, s, _ in res]


@pytest.mark.parametrize("dim", [132, 768, 2052])
def test_one_example_is_the_search(dim):
    idx, raw, _ = _index(3001, dim, seed=dim)
    mask = np.random.RandomState(dim).rand(3001) < 0.3
    f = idx.make_filter(mask)
    for j, q in enumerate(orc.synth_queries(4, dim, seed=dim + 1)):
        for k, eta, pref in ((10, 0.5, 0.0), (40, 0.3, 0.2)):
            want = idx.search(q, k, eta, pref)
            assert _pairs(idx.search_by_examples([q], k=k, eta=eta, entropy_pref=pref)) == _pairs(want), (j, k)
            want = idx.search(q, k, eta, pref, filter=f)
            assert _pairs(idx.search_by_examples([q], k=k, eta=eta, entropy_pref=pref, filter=f)) == _pairs(want), (j, k, "filter")
    # a stored row by id, not excluded, is the search for that row
    want = idx.search(idx._stored_rows()[17], 10, 0.5, 0.0)
    assert _pairs(idx.search_by_examples(["d17"], k=10, exclude_examples=False)) == _pairs(want)


# ------------------------------------------------------------------------------------------------------ 4. exclusion, filter
def test_examples_by_id_exclusion_and_rules():
    idx, raw, _ = _index(2000, 256, seed=3)
    pos, neg = ["d5", "d900", raw[40] * 2], ["d77"]
    res = idx.search_by_examples(pos, neg, k=30, eta=0.0)
    got = [d for d, _, _ in res]
    assert len(got) == 30 and not {"d5", "d900", "d77"} & set(got) and "d40" in got       # the vector's own row is not excluded
    res = idx.search_by_examples(pos, neg, k=30, eta=0.0, exclude_examples=False)
    assert {d for d, _, _ in res[:3]} == {"d5", "d900", "d40"} and "d77" not in [d for d, _, _ in res]
    assert idx.search_by_examples(["d5"], k=1, eta=0.0, exclude_examples=False)[0][0] == "d5"
    with pytest.raises(KeyError):
        idx.search_by_examples(["d5", "nope"])
    assert idx.search_by_examples(pos, k=0) == [] and idx.search_by_examples(pos, k=5, filter=np.zeros(2000, bool)) == []
    # k against the rows OFFERED: 2000 rows less two excluded documents; a filter of 6 rows, one of them an example
    assert len(idx.search_by_examples(["d5", "d900"], k=1998, candidates=1998)) == 1998
    with pytest.raises(ValueError):
        idx.search_by_examples(["d5", "d900"], k=1999, candidates=1999)
    few = idx.make_filter(rows=np.array([5, 6, 7, 8, 9, 10]))
    assert len(idx.search_by_examples(["d5"], k=5, filter=few)) == 5
    with pytest.raises(ValueError):
        idx.search_by_examples(["d5"], k=6, filter=few)
    assert len(idx.search_by_examples(["d5"], k=6, filter=few, exclude_examples=False)) == 6
    with pytest.raises(ValueError, match="2048"):
        idx.search_by_examples(["d5"], k=10, candidates=2049)
    # a Where predicate and a dedup filter are filters like any other
    keep = idx.dedup_filter(0.99)
    assert len(idx.search_by_examples(pos, neg, k=5, filter=keep)) == 5
    # stale filter
    from dewi.types import Payload
    idx.add("extra", raw[0], Payload())
    idx.build()
    with pytest.raises(ValueError):
        idx.search_by_examples(["d5"], k=5, filter=few)


def test_unsupported_corpora_raise_value_error():
    from dewi.backends import ExactIndex
    from dewi.types import payloads_from_columns
    for dim, space, word in ((128, "cosine", "132"), (134, "cosine", "% 4"), (256, "l2", "cosine")):
        raw = orc.synth_corpus(100, dim, seed=1)
        idx = ExactIndex(dim, space)
        idx.add_batch([f"d{i}" for i in range(100)], raw, payloads_from_columns(orc.synth_payload_columns(100, seed=1)))
        with pytest.raises(ValueError, match=word.replace("%", "%")):
            idx.search_by_examples([raw[0]], k=5)
    c, _, _, _ = _corpus("gauss", 100, 256, seed=2)
    with pytest.raises(ValueError, match="fp32"):
        c.to_bf16().candidates_examples_device(torch.zeros((1, 256), device=c.device), 1, 5)


@pytest.mark.parametrize("dim", [132, 768, 1000])
def test_list_form_is_the_dense_form_on_the_reduced_corpus(dim):
    n = 1601
    c, raw, dewi32, ent32 = _corpus("gauss", n, dim, seed=dim + 9, id_offset=1000)
    pool = _example_pool("gauss", raw, seed=dim + 10)
    X = _request(pool, 3, 2)
    rs = np.random.RandomState(dim)
    mask = rs.rand(n) < 0.35
    mask[[DUP_FIRST, DUP_FIRST + 1, ZERO_ROW]] = True
    rows = np.flatnonzero(mask)
    f = c.make_filter(mask)
    sub = _eng().DeviceCorpus(c.emb[torch.from_numpy(rows).to(c.device)].contiguous(), c.dewi32[torch.from_numpy(rows).to(c.device)],
                              c.ent32[torch.from_numpy(rows).to(c.device)], "cosine")
    S = _sims(c, X, f)
    assert np.isnan(S[:, ~mask]).all()
    excl_in, excl_out = int(rows[7]), int(np.flatnonzero(~mask)[3])
    for cut in (10, 100, 300, 2048):                          # 2048 > |A|: padding behind the list's rows
        for exclude in (None, [excl_in, excl_out, excl_in]):
            got = _call(c, X, 3, cut, "any", "penalty", 1.0, exclude=exclude, filt=f)
            sub_ex = None if exclude is None else [int(np.searchsorted(rows, excl_in))]
            red = _call(sub, X, 3, cut, "any", "penalty", 1.0, exclude=sub_ex)
            m = min(cut, rows.size - (1 if exclude else 0))
            assert (got["id"][m:] == -1).all() and (red["id"][m:] == -1).all() and (got["id"][:m] >= 1000).all()
            assert np.array_equal(got["id"][:m] - 1000, rows[red["id"][:m]])
            for fld in ("sim", "dewi", "ent"):
                assert np.array_equal(got[fld].view(np.uint32), red[fld].view(np.uint32)), (cut, fld)
            score = xm.combine(S, 3)[rows]
            _same_records(got, xm.records(score, rows, dewi32, ent32, cut, exclude or (), 1000), (dim, cut))
            if exclude:
                assert excl_in + 1000 not in got["id"]
    # an empty filter: DEWI_OK, nothing launched, nothing written
    empty = c.make_filter(np.zeros(n, bool))
    assert _call(c, X, 3, 10, filt=empty, writes=False, override=dict(d_ws=None, ws_bytes=0)) is None
    recs = c.candidates_examples_device(torch.from_numpy(X).to(c.device), 3, 10, filter=empty)
    assert (_eng().records_to_numpy(recs)["id"] == -1).all()


def test_device_methods_use_the_cache_and_check_stale_filters():
    c, raw, dewi32, ent32 = _corpus("emb", 1500, 388, seed=4)
    other, _, _, _ = _corpus("emb", 1500, 388, seed=5)
    pool = _example_pool("emb", raw, seed=6)
    X = _request(pool, 2, 1)
    x = torch.from_numpy(X).to(c.device)
    S = _sims(c, X)
    recs = c.candidates_examples_device(x, 2, 50, negative_weight=0.5)
    assert ("examples", 1500, 50) in c.cached_workspaces()
    wsguard.guard(c)
    wsguard.poison(c, "0xff")
    again = c.candidates_examples_device(x, 2, 50, negative_weight=0.5)
    wsguard.check(c, interior=False)
    wsguard.release(c)
    want = xm.records(xm.combine(S, 2, negative_weight=0.5), None, dewi32, ent32, 50)
    _same_records(_eng().records_to_numpy(recs)[0], want, "cached")
    _same_records(_eng().records_to_numpy(again)[0], want, "poisoned cache")
    ids, sc = c.search_examples_device(x, 2, 10, 0.3, 0.1, negative_weight=0.5)
    mi, ms = xm.search(xm.combine(S, 2, negative_weight=0.5), None, dewi32, ent32, 20, 10, 0.3, 0.1)
    assert np.array_equal(ids.cpu().numpy()[0], mi) and np.array_equal(sc.cpu().numpy()[0].view(np.uint32), ms.view(np.uint32))
    with pytest.raises(ValueError):
        c.candidates_examples_device(x, 2, 50, filter=other.make_filter(np.ones(1500, bool)))
    with pytest.raises(ValueError):
        c.search_examples_device(x, 2, 1501, 0.3, 0.0)


def test_facade_and_ivf_forward():
    from dewi.index import DewiIndex
    from dewi.ivf import IVFIndex
    from dewi.types import payloads_from_columns
    n, d = 1200, 256
    raw = orc.synth_corpus(n, d, seed=8)
    cols = orc.synth_payload_columns(n, seed=8)
    index = DewiIndex(dim=d, use_ann=False, rerank_eta=0.3)
    index.add_batch([f"d{i}" for i in range(n)], raw, payloads_from_columns(cols))
    exact, _, _ = _index(n, d, seed=8)
    a = index.search_by_examples(["d3", raw[9]], ["d100"], k=7, negative_rule="best_score")
    b = exact.search_by_examples(["d3", raw[9]], ["d100"], k=7, eta=0.3, negative_rule="best_score")
    assert _pairs(a) == _pairs(b) and len(a) == 7
    ivf, _, _ = _index(n, d, seed=8, cls=IVFIndex, nlist=8)
    assert _pairs(ivf.search_by_examples(["d3", raw[9]], ["d100"], k=7, eta=0.3, negative_rule="best_score")) == _pairs(b)


# ------------------------------------------------------------------------------------------------------ 5. ABI errors
def test_abi_errors_write_nothing():
    nat = _nat()
    c, raw, _, _ = _corpus("gauss", 500, 256, seed=1)
    X = _request(_example_pool("gauss", raw, seed=2), 2, 1)
    f = c.make_filter(np.arange(500) % 2 == 0)
    INV, UNS, WS = nat.ERR_INVALID_ARG, nat.ERR_UNSUPPORTED, nat.ERR_WORKSPACE
    bad = [
        (INV, dict(d_E=None)), (INV, dict(d_x=None)), (INV, dict(d_dewi=None)), (INV, dict(d_ent=None)), (INV, dict(d_out=None)),
        (INV, dict(n_rows=0)), (INV, dict(dim=0)), (INV, dict(dim=-256)), (UNS, dict(n_rows=1 << 32)),
        (INV, dict(n_pos=0)), (INV, dict(n_pos=-1)), (INV, dict(n_neg=-1)), (UNS, dict(n_pos=9, n_neg=8)), (UNS, dict(n_pos=17, n_neg=0)),
        (INV, dict(match=2)), (INV, dict(match=-1)), (INV, dict(rule=2)), (INV, dict(rule=-1)),
        (INV, dict(w=float("nan"))), (INV, dict(w=float("inf"))), (INV, dict(w=-float("inf"))), (INV, dict(w=1e39)),
        (INV, dict(n_ex=-1)), (INV, dict(n_ex=17)), (INV, dict(n_ex=2, d_ex=None)),
        (INV, dict(cut=0)), (INV, dict(cut=-3)), (UNS, dict(cut=2049)),
        (UNS, dict(dim=128)), (UNS, dict(dim=64)), (UNS, dict(dim=254)), (UNS, dict(dim=4100)),
        (UNS, dict(id_offset=-1)), (UNS, dict(id_offset=(1 << 31) - 400)),
        (WS, dict(d_ws=None)), (WS, dict(ws_bytes=0)),
    ]
    for code, override in bad:
        assert _call(c, X, 2, 20, expect=code, override=override) is None, override
    need = int(c._lib.dewi_knn_examples_workspace_bytes(500, 256, 3, 20))
    assert _call(c, X, 2, 20, expect=WS, override=dict(ws_bytes=need - 1)) is None
    for n_allowed in (-1, 501):
        assert _call(c, X, 2, 20, filt=f, expect=INV, override=dict(n_allowed=n_allowed)) is None
    assert _call(c, X, 2, 20, filt=f, writes=False, override=dict(n_allowed=0, d_ws=None, ws_bytes=0)) is None   # DEWI_OK, nothing written
    assert _call(c, X, 2, 20, filt=f) is not None                                                 # and the call as it should be works


# ------------------------------------------------------------------------------------------------------ 6. oracle
def _oracle_check(E, X, n_pos, match, rule, w, dewi32, ent32, k, eta, pref, got_ids, got_sc):
    """tests/parity.py's rule (GAP = 5e-7, scores within 1e-5 of the magnitude; decisive queries id for id, near ties by the
    admissible-outcome check) with the combined score in the similarity's place.  Returns whether the query was decisive."""
    n = E.shape[0]
    s32 = xm.combine((xm.prepare_examples(X) @ E.T).astype(F), n_pos, match, rule, w)
    s64 = xm.combine64(xm.similarities64(E, X), n_pos, match, rule, w)
    assert not np.isnan(s64).any()
    c = min(2 * k, n)
    ref_ids, ref_sc = xm.search(s32, None, dewi32, ent32, c, k, eta, pref)
    adj64 = np.float64(F(1 - eta)) * s64 + np.float64(F(eta)) * dewi32.astype(np.float64)
    if pref != 0:
        adj64 = adj64 + np.float64(F(pref)) * ent32.astype(np.float64)
    s_key, v_c, v_c1, cut_gap, rank_gap, scale, g_cut, g, decisive = parity._decision(s64, adj64, np.zeros(n, bool), ref_sc, k, eta,
                                                                                       parity.GAP)
    gi = np.asarray(got_ids, dtype=np.int64)
    assert gi.shape == ref_ids.shape and gi.min() >= 0 and gi.max() < n and len(set(gi.tolist())) == gi.size
    assert np.all(got_sc[:-1] >= got_sc[1:]), "scores not non-increasing"
    if decisive:
        assert np.array_equal(gi, ref_ids), (gi.tolist(), ref_ids.tolist(), cut_gap, rank_gap)
        assert np.max(np.abs(got_sc.astype(np.float64) - ref_sc.astype(np.float64))) <= parity.SCORE_TOL * scale
        return True
    assert np.all(s_key[gi] >= v_c - g_cut), "a returned row is not among the top-c combined scores"
    want = parity._row_scores32(s32, gi, dewi32, ent32, eta, pref)
    assert np.max(np.abs(got_sc.astype(np.float64) - want.astype(np.float64))) <= parity.SCORE_TOL * scale
    sure = s_key > v_c1 + g_cut if c < n else np.ones(n, bool)
    sure[gi] = False
    assert not np.any(adj64[sure] > float(np.min(adj64[gi])) + g), "a sure candidate that beats the worst returned score was left out"
    return False


@pytest.mark.parametrize("dim", [388, 1536])
def test_against_the_float64_oracle(dim):
    n, k, eta, pref = 4001, 10, 0.3, 0.1
    c, raw, dewi32, ent32 = _corpus("gauss", n, dim, seed=dim + 21)
    E = c.emb.cpu().numpy()
    keep = np.ones(n, bool)
    keep[ZERO_ROW] = False                                                     # (the NaN row: the bit-parity tests' business)
    mask = (np.random.RandomState(dim).rand(n) < 0.4) & keep
    total = dec = 0
    for t in range(4):
        pool = _example_pool("gauss", raw[keep], seed=dim + 30 + t)
        for (n_pos, n_neg), match, rule, w in (((3, 1), "any", "penalty", 1.0), ((2, 3), "any", "best_score", 1.0),
                                               ((5, 0), "all", "penalty", 1.0), ((8, 8), "any", "penalty", 0.5)):
            X = _request(pool, n_pos, n_neg)
            x = torch.from_numpy(X).to(c.device)
            for allowed in (keep, mask):
                rows = np.flatnonzero(allowed)
                ids, sc = c.search_examples_device(x, n_pos, k, eta, pref, match=match, negative_rule=rule, negative_weight=w,
                                                   filter=c.make_filter(allowed))
                ids, sc = ids.cpu().numpy()[0], sc.cpu().numpy()[0]
                pos = np.searchsorted(rows, ids)
                assert np.array_equal(rows[np.minimum(pos, rows.size - 1)], ids), "an id outside the filter"
                dec += _oracle_check(E[rows], X, n_pos, match, rule, w, dewi32[rows], ent32[rows], k, eta, pref, pos, sc)
                total += 1
    assert dec >= 0.5 * total, f"only {dec}/{total} decisive requests"

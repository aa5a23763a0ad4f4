"""GPU parity tests of every matrix-core search route on corpora arranged against its sampler (tests/corpora.py).

The other parity tests search i.i.d. Gaussian rows: a query's survivors spread evenly over the workgroups of the filter pass
and no query is ever refused.  Here

* ``planted_runs`` puts a run of D graded near-copies of every query's base row into the tiles of ONE workgroup, with D
  sweeping 1 .. d_max across the batch: the survivor segment of (workgroup, query) is below, at and above its capacity
  (``plan_mfma_f32``: 16 records at 66 000 rows and c = 20; ``plan_mfma``: 32 per quarter-segment) for different queries of
  one call, so one batch mixes refused and served queries;
* ``embedding_like`` crowds all scores into a narrow band below 1 (every pair of rows has a cosine of 0.45 .. 1).

Per route the test first asserts that the library takes it (``scan_kernel_name``; on the shadow routes that the call has
refusal flags at all), then:

  1. ``search_device`` returns no id -1 and no NaN score;
  2. ``check_batch`` against the oracle for (up to) 32 queries spread over the sweep, floor 0.75 (a condition on the inputs
     that tests/test_corpora_host.py checks on the CPU), the tolerances those routes already use;
  3. every query ``refused_by_last_call`` names is bit-equal, ids and scores, to the one-query search on the row kernels;
  4. not vacuous: at least 3 planted queries were refused and at least 3 were not, and (routes a, b, d) both kinds occur
     inside one group of 32 consecutive queries;
  5. the same call again, and again after a call of another batch size and k on the same corpus (workspaces reused), gives
     bit-equal outputs.

Route (c), 1024 columns, has 8 queries, all planted, all checked by the oracle (its sweep is 1, 2, 5, 10, 21, 44, 94, 200).

FIRST REFUSED RUN LENGTH per route: NOT MEASURED on the hardware yet.  Every planted case prints it (``pytest -s``: "first
refused D = ..., longest served D = ..., refused n of b"); from the capacity formulas and the tile layout it should be 17 on the
depth-split routes at c = 20 (a segment holds 16 records; D = 14 .. 16 only with stray survivors of the ~0.6 per segment a
Gaussian corpus leaves), about 56 there at c = 200 and 131 072 rows (63 records, ~8 strays), and on the 256-query kernel 129 or
less (a quarter-segment holds 32 records and gets 8 rows of every tile: 128 rows fill all four, D = 116 fills quarter 0 to
exactly 32 and is refused only with a stray), about 104 at c = 200 (~6 strays per quarter).  Assertion 4 holds for any first
refused D between 11 and 44 (depth-split, c = 20) and up to 152 (256-query kernel).
"""
import ctypes

import numpy as np
import pytest

import corpora
import dewi_oracle as orc
from parity import check_batch, device_prepared_queries

pytestmark = pytest.mark.gpu

ETA, PREF = 0.3, 0.1
FLOOR = 0.75
# bf16 corpora: the oracle runs on the stored bf16 rows and the device's prepared queries (tests/test_hip_mfma.py TOL)
TOL_BF16 = dict(gap=1e-6, score_tol=1e-5, prepared=True, exact_gaps=False)
TOL_F32 = dict(exact_gaps=False)

_host = {}


def _owners(n):
    from dewi import _native as nat
    cus = ctypes.c_int(0)
    nat.check(nat.load_library().dewi_device_info(ctypes.byref(cus), None, None))
    return min((n + corpora.TILE_ROWS - 1) // corpora.TILE_ROWS, int(cus.value))


def _planted(name):
    """The planted corpus of a case, made once per session and never written to."""
    n, dim, b, k, d_max = corpora.PLANTED_CASES[name]
    key = (name, _owners(n))
    if key not in _host:
        X, Q, D, rows = corpora.planted_runs(n, dim, b, seed=dim + b, d_max=d_max, owners=key[1])
        cols = orc.synth_payload_columns(n, seed=dim + b)
        for a in (Q, D):                               # (X goes to torch.from_numpy, which wants a writable array; nobody writes to it)
            a.flags.writeable = False
        _host[key] = (X, Q, D, cols)
    return _host[key] + (k,)


def _embedding():
    n, dim, nq, seed = corpora.EMBEDDING_CASE
    if "emb" not in _host:
        X, Q, _, q_rows = corpora.embedding_like(n, dim, seed, n_queries=nq)
        cols = orc.synth_payload_columns(n, seed=seed)
        for a in (Q, q_rows):
            a.flags.writeable = False
        _host["emb"] = (X, Q, q_rows, cols)
    return _host["emb"]


def _device(X, cols, kind, id_offset=0):
    """kind: 'bf16' | 'f32' | 'l2' (fp32 rows, unnormalised) | 'shadow' (fp32 + bf16 shadow, one-query searches too)."""
    from dewi import _engine as eng
    c = eng.DeviceCorpus.from_host(X, cols["dewi"], cols["ht_mean"], cols["hi_mean"], space="l2" if kind == "l2" else "cosine",
                                   id_offset=id_offset)
    if kind == "bf16":
        c = c.to_bf16()
    if kind == "shadow":
        c.enable_bf16_shadow(single_query=True)
    return c


def _oracle_matrix(c):
    return (c.emb.float() if c.is_bf16 else c.emb).cpu().numpy()


def _assert_route(c, kind, b, k, prefix):
    """The library really takes the route under test for a batch of ``b``."""
    from dewi import _native as nat
    if kind != "shadow":
        name = c.scan_kernel_name(b, k)
        assert name.startswith(prefix), (name, prefix)
        return
    off = ctypes.c_size_t(0)
    nat.check(c._lib.dewi_knn_refusal_flags(0, 1, c.n_rows, c.dim, b, k, min(2 * k, c.n_rows), nat.SPACE_CODES[c.space],
                                            ctypes.byref(off)))
    assert off.value != ctypes.c_size_t(-1).value, "this shape does not go through the shadow: no refusal flags"


def _search(c, q_dev, k, eta=ETA, pref=PREF):
    ids_d, sc_d = c.search_device(q_dev, k, eta, pref)
    refused = c.refused_by_last_call()             # (synchronises; reads the flags of THIS call's workspace)
    return ids_d.cpu().numpy(), sc_d.cpu().numpy(), refused


def _check_route(c, cols, kind, Q, k, eta=ETA, pref=PREF, other=(7, 3), label=""):
    """Assertions 1, 2, 3 and 5 for one batch; returns (refused bool [b], ids, scores)."""
    import torch
    b = Q.shape[0]
    space = "l2" if kind == "l2" else "cosine"
    q_dev = torch.from_numpy(np.array(Q, dtype=np.float32)).cuda()
    ids, sc, refused = _search(c, q_dev, k, eta, pref)
    print(f"{label}: {int(refused.sum())} of {b} queries refused")
    # 1. always answered
    assert ids.min() >= 0 and not np.isnan(sc).any()
    # 2. the oracle
    sel = corpora.oracle_queries(b)
    E = _oracle_matrix(c)
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    if c.is_bf16:
        check_batch(E, device_prepared_queries(Q[sel], space), dewi32, ent32, k, eta, pref, space, ids[sel], sc[sel],
                    min_decisive_frac=FLOOR, **TOL_BF16)
    else:
        check_batch(E, Q[sel], dewi32, ent32, k, eta, pref, space, ids[sel], sc[sel], min_decisive_frac=FLOOR, **TOL_F32)
    # 3. a refused query was answered by the row kernels: bit-equal to its one-query search (shadow corpora: the one-query
    #    search of the fp32 rows, which every shadow route equals bit for bit — so a few served queries are compared as well)
    singles = np.flatnonzero(refused).tolist()
    if kind == "shadow":
        singles += np.flatnonzero(~refused)[:: max(1, b // 8)].tolist()
    for j in singles:
        one_ids, one_sc = c.search_device(q_dev[j:j + 1].contiguous(), k, eta, pref, use_shadow=False)
        assert not c.refused_by_last_call().any()
        assert np.array_equal(ids[j], one_ids.cpu().numpy()[0]) and np.array_equal(sc[j], one_sc.cpu().numpy()[0]), \
            f"query {j} ({'refused' if refused[j] else 'served'}) differs from its one-query search"
    # 5. repeatable: the same call again, and again after another batch size and k went through the same corpus object
    ids2, sc2, refused2 = _search(c, q_dev, k, eta, pref)
    assert np.array_equal(ids2, ids) and np.array_equal(sc2, sc) and np.array_equal(refused2, refused)
    ob, ok = other
    o_ids, o_sc = c.search_device(q_dev[:min(ob, b)].contiguous() if b > 1 else q_dev.repeat(ob, 1), ok, eta, pref)
    assert o_ids.min().item() >= 0
    ids3, sc3, refused3 = _search(c, q_dev, k, eta, pref)
    assert np.array_equal(ids3, ids) and np.array_equal(sc3, sc) and np.array_equal(refused3, refused)
    return refused, ids, sc


def _assert_not_vacuous(refused, D, label, one_group):
    """Assertion 4.  Prints the record FIRST_REFUSED keeps."""
    D = np.asarray(D)
    n_ref = int(refused.sum())
    first = int(D[refused].min()) if n_ref else None
    last_served = int(D[~refused].max()) if n_ref < refused.size else None
    print(f"{label}: first refused D = {first}, longest served D = {last_served}, refused {n_ref} of {refused.size}; "
          f"refused D = {sorted(set(D[refused].tolist()))}")
    assert n_ref >= 3 and refused.size - n_ref >= 3, f"{label}: {n_ref} refused, {refused.size - n_ref} served"
    if one_group:
        mixed = [g for g in range(0, refused.size, 32) if refused[g:g + 32].any() and not refused[g:g + 32].all()]
        assert mixed, f"{label}: no group of 32 consecutive queries holds both refused and served ones"


# route: (case, kind, kernel prefix, refused and served must share a group of 32)
PLANTED_ROUTES = {
    "a-bf16-256query": ("n66000-d256-b40", "bf16", "mfma_scan_bf16_s16", True),
    "b-bf16-depth": ("n66000-d256-b32", "bf16", "mfma_scan_f32<true", True),
    "c-bf16-depth-1024": ("n65600-d1024-b8", "bf16", "mfma_scan_f32<true", False),
    "d-f32-whole-chunk": ("n66000-d256-b32", "f32", "mfma_scan_f32<false", True),
    "e-f32-partial-chunk": ("n66000-d128-b32", "f32", "mfma_scan_f32<false", False),
    "f-f32-l2-refine": ("n66000-d256-b12", "l2", "mfma_scan_f32<false", False),
    "g-shadow-b256": ("n66000-d256-b256", "shadow", None, False),
    "g-shadow-b40": ("n66000-d256-b40", "shadow", None, False),
    "g-shadow-b8": ("n66000-d256-b8", "shadow", None, False),
    "h-bf16-256query-k100": ("n131072-d256-b40-k100", "bf16", "mfma_scan_bf16_s16", True),
    "h-f32-k100": ("n131072-d256-b32-k100", "f32", "mfma_scan_f32<false", True),
}


@pytest.mark.parametrize("route", list(PLANTED_ROUTES))
def test_planted_runs_refused_and_served_in_one_batch(route):
    case, kind, prefix, one_group = PLANTED_ROUTES[route]
    X, Q, D, cols, k = _planted(case)
    c = _device(X, cols, kind)
    _assert_route(c, kind, Q.shape[0], k, prefix)
    refused, _, _ = _check_route(c, cols, kind, Q, k, label=route)
    _assert_not_vacuous(refused, D, route, one_group)


def test_planted_runs_one_query_through_the_shadow_lists():
    """One query over an fp32 corpus with a bf16 shadow (``single_query=True``): the bf16 row kernel with per-workgroup lists
    + the exact re-scoring, for the shortest, a middle and the longest run of the sweep.  Whether the list route refuses is
    printed, not asserted (three queries); what is asserted is that each is answered as the fp32 row kernels answer it."""
    X, Q, D, cols, k = _planted("n66000-d256-b8")
    c = _device(X, cols, "shadow")
    _assert_route(c, "shadow", 1, k, None)
    for j in (0, 4, 7):                                  # D = 1, 21, 200
        refused, ids, _ = _check_route(c, cols, "shadow", Q[j:j + 1], k, other=(8, 3), label=f"lists D={int(D[j])}")
        print(f"lists D={int(D[j])}: refused {bool(refused[0])}")


@pytest.mark.parametrize("route", ["a-bf16-256query", "d-f32-whole-chunk"])
def test_planted_runs_pipelined_equals_the_one_call_search(route):
    """dewi_knn_scan / dewi_knn_finish with three workspaces in rotation: a batch with refused queries, the same batch in
    reverse order (the refused queries at other positions of their waves) and the first again, twice round — every result
    bit-equal to the one-call search, every query answered (the repair runs inside dewi_knn_finish)."""
    import torch
    from dewi import _engine as eng
    case, kind, prefix, _ = PLANTED_ROUTES[route]
    X, Q, D, cols, k = _planted(case)
    c = _device(X, cols, kind)
    b = Q.shape[0]
    _assert_route(c, kind, b, k, prefix)
    q_dev = torch.from_numpy(np.stack([Q, Q[::-1], Q])).cuda()
    want, n_refused = [], []
    for i in range(3):
        ids_d, sc_d = c.search_device(q_dev[i], k, ETA, PREF)
        n_refused.append(int(c.refused_by_last_call().sum()))
        want.append((ids_d.clone(), sc_d.clone()))
    assert min(n_refused) >= 3, n_refused                # the pipeline has something to repair in every batch
    assert torch.equal(want[1][0], want[0][0].flip(0)) and torch.equal(want[1][1], want[0][1].flip(0))   # position-independent
    pipe = eng.PipelinedSearcher(c, k, ETA, PREF, n_queries=b, depth=3)
    ids = torch.full((6, b, k), -7, dtype=torch.int64, device="cuda")
    sc = torch.full((6, b, k), float("nan"), dtype=torch.float32, device="cuda")
    for i in range(6):
        pipe.submit(q_dev[i % 3], ids[i], sc[i])
    pipe.drain()
    for i in range(6):
        assert torch.equal(ids[i], want[i % 3][0]) and torch.equal(sc[i], want[i % 3][1]), f"submit {i}"
    recs = torch.empty((b, 2 * k, 4), dtype=torch.int32, device="cuda")
    pipe2 = eng.PipelinedSearcher(c, k, ETA, PREF, n_queries=b, n_candidates=2 * k, depth=3)
    pipe2.submit(q_dev[0], out_records=recs)
    pipe2.drain()
    assert (recs[:, :, 3] >= 0).all().item()             # no refusal marker leaves the library
    assert torch.equal(recs, c.candidates_device(q_dev[0], 2 * k))


@pytest.mark.parametrize("route", ["a-bf16-256query", "d-f32-whole-chunk"])
def test_planted_runs_in_two_shards_merge_to_the_oracle(route):
    """140 000 rows in two shards of whole tiles (70 016 + 69 984 rows, both matrix-core shapes), each with planted runs of
    its own — the first half of the batch has its runs in shard 0, the second half in shard 1, whose records carry the id
    offset: ``candidates_device`` per shard (refused queries repaired inside the call, no marker in any record), then
    ``merge_rerank_device``, against the oracle on the whole corpus."""
    import torch
    from dewi import _engine as eng
    _, kind, prefix, _ = PLANTED_ROUTES[route]
    b, k, dim, d_max = (40 if kind == "bf16" else 32), 10, 256, 256
    sizes = (70_016, 69_984)
    key = ("shards", b, _owners(sizes[0]))
    if key not in _host:
        parts = [corpora.planted_runs(n_s, dim, b // 2, seed=900 + s, d_max=d_max, owners=_owners(n_s)) for s, n_s in enumerate(sizes)]
        X = np.concatenate([p[0] for p in parts])
        Q = np.concatenate([p[1] for p in parts])
        Q.flags.writeable = False
        _host[key] = (X, Q, orc.synth_payload_columns(X.shape[0], seed=900))
    X, Q, cols = _host[key]
    q_dev = torch.from_numpy(np.array(Q)).cuda()
    lists, E = [], []
    for s, (lo, hi) in enumerate(((0, sizes[0]), (sizes[0], sizes[0] + sizes[1]))):
        sh = _device(X[lo:hi], {key_: v[lo:hi] for key_, v in cols.items()}, kind, id_offset=lo)
        _assert_route(sh, kind, b, k, prefix)
        recs = sh.candidates_device(q_dev, 2 * k)
        refused = sh.refused_by_last_call()
        own = slice(s * (b // 2), (s + 1) * (b // 2))      # the queries whose runs lie in this shard
        print(f"{route} shard {s}: refused {np.flatnonzero(refused).tolist()}")
        assert refused[own].any() and not refused[own].all()     # something to repair in this shard, and something served
        ids_s = recs[:, :, 3].cpu().numpy()
        assert ids_s.min() >= lo and ids_s.max() < hi        # real rows of this shard, offset applied; no marker (-2)
        for j in np.flatnonzero(refused)[:4]:                # the repair's records == the row kernels' records
            assert torch.equal(recs[j], sh.candidates_device(q_dev[j:j + 1].contiguous(), 2 * k)[0])
        lists.append(recs)
        E.append(_oracle_matrix(sh))
    ids_d, sc_d = eng.merge_rerank_device(torch.stack(lists), 2 * k, k, ETA, PREF)
    ids, sc = ids_d.cpu().numpy(), sc_d.cpu().numpy()
    assert ids.min() >= 0 and not np.isnan(sc).any()
    dewi32, ent32 = orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])
    sel = corpora.oracle_queries(b)
    if kind == "bf16":
        check_batch(np.concatenate(E), device_prepared_queries(Q[sel]), dewi32, ent32, k, ETA, PREF, "cosine", ids[sel], sc[sel],
                    min_decisive_frac=FLOOR, **TOL_BF16)
    else:
        check_batch(np.concatenate(E), Q[sel], dewi32, ent32, k, ETA, PREF, "cosine", ids[sel], sc[sel], min_decisive_frac=FLOOR,
                    **TOL_F32)


EMBEDDING_ROUTES = {
    "a-bf16-256query": ("bf16", 40, 10, "mfma_scan_bf16_s16"),
    "d-f32-whole-chunk": ("f32", 40, 10, "mfma_scan_f32<false"),        # two passes of the depth-split kernel
    "g-shadow-b40": ("shadow", 40, 10, None),
    "a-bf16-256query-k100": ("bf16", 40, 100, "mfma_scan_bf16_s16"),
}


@pytest.mark.parametrize("route", list(EMBEDDING_ROUTES))
def test_embedding_like_scores_crowded_below_one(route):
    """Anisotropic clustered rows: every score of a query lies in 0.45 .. 1, the sample threshold and the shadow margin have
    the least room.  Assertions 1, 2, 3, 5; and at eta = 0 the four queries that ARE corpus rows find their own row first with
    the score blend(1.0, ...) = the self-similarity (bf16: of the stored bf16 row and the prepared query)."""
    import torch
    kind, b, k, prefix = EMBEDDING_ROUTES[route]
    X, Q, q_rows, cols = _embedding()
    Q = Q[:b]
    c = _device(X, cols, kind)
    _assert_route(c, kind, b, k, prefix)
    _check_route(c, cols, kind, Q, k, label=f"embedding {route}")
    if k == 10:
        refused, ids, sc = _check_route(c, cols, kind, Q, k, eta=0.0, pref=0.0, label=f"embedding {route} eta 0")
        assert ids[:4, 0].tolist() == q_rows[:4].tolist()
        if kind == "bf16":
            Eb, Qp = _oracle_matrix(c), device_prepared_queries(np.array(Q[:4]))
            want = np.einsum("qd,qd->q", Eb[q_rows[:4]].astype(np.float64), Qp.astype(np.float64))
        else:
            want = np.ones(4)
        assert np.max(np.abs(sc[:4, 0] - want)) <= 1e-5, sc[:4, 0]

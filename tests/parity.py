"""Parity harness shared by the GPU tests: HIP result vs the CPU oracle.

Rule (SURVEY.md §8(a) note 5): fp32 dot products are summed in a different order by OpenBLAS
and by the GPU (~1e-7 relative), so a query is compared in one of two ways.

* DECISIVE query — the similarity gap at the candidate cut and the smallest adjacent
  adjusted-score gap among ranks 1..k+1 (both computed in float64) exceed GAP (5e-7, scaled by
  the score magnitude for l2): the id ranking must EQUAL the oracle's, scores within 1e-5.
* near-tie query — an admissible-outcome check that still compares ids, not just scores:
  (a) every returned row is an admissible candidate (its f64 similarity is not below the c-th
      best by more than GAP),
  (b) every returned score equals the oracle's fp32 blend FOR THAT ROW within the tolerance
      (this pins the id <-> score pairing),
  (c) no row that is surely a candidate (similarity above the first excluded row by more than
      GAP) and beats the worst returned adjusted score by more than GAP was left out,
  (d) no duplicates, scores non-increasing.
  So the returned id SET can differ from the oracle's only in rows within GAP of a decision
  boundary, and the order only between rows whose adjusted scores are within the tolerance.

NaN adjusted scores (zero-norm rows of a cosine corpus, NaN rows, NaN payload values, 0 * inf): the reference keeps such
rows in the cut and in the top k (NaN sorts as the largest value in argpartition) and returns them LAST (argsort of the
negated scores, backends.py:468-471).  Both kinds of query therefore require the NaN scores of a result to be its tail and
the ids of the tail to be the oracle's NaN candidates as a set whenever they all fit into k (the order inside the tail is
an introselect artefact in the reference); the rules above apply to the numbers in front of the tail, with the gaps taken
over the candidates whose adjusted score is a number.  A query with NaN rows can be decisive.

``check_batch`` returns the decisive count and asserts a floor on it (default: 80 % of the
queries at k <= 10, 25 % above): no case can pass on near-tie checks alone.
"""
import numpy as np

import dewi_oracle as orc

GAP = 5e-7
SCORE_TOL = 1e-5


def _reference(E, q, dewi32, ent32, k, eta, pref, space, exact_gaps, prepared):
    """Oracle result + the float64 companion quantities the near-tie rules need."""
    qp = np.asarray(q, dtype=np.float32) if prepared else orc.prepare_query(q, space)
    s32 = orc.similarities(E, qp, space)                                   # backends.py:431-436
    cand = orc.candidate_cut(s32, k)
    if cand.size:
        ref_ids, ref_sc = orc.rerank(cand, s32[cand], dewi32, ent32, k, eta, pref)
    else:
        ref_ids, ref_sc = np.empty(0, np.int64), np.empty(0, np.float32)
    if exact_gaps:
        q64 = qp.astype(np.float64)
        E64 = E.astype(np.float64)
        s64 = E64 @ q64 if space != "l2" else -np.sum((E64 - q64[None, :]) ** 2, axis=1)
    else:
        s64 = s32.astype(np.float64)
    w_sim, w_dewi, w_ent = np.float64(np.float32(1 - eta)), np.float64(np.float32(eta)), np.float64(np.float32(pref))
    with np.errstate(invalid="ignore"):          # 0 * inf, inf - inf: NaN scores are part of the contract
        adj64 = w_sim * s64 + w_dewi * dewi32.astype(np.float64)
        if pref != 0:
            adj64 = adj64 + w_ent * ent32.astype(np.float64)
    return s32, s64, adj64, ref_ids, ref_sc


def _row_scores32(s32, rows, dewi32, ent32, eta, pref):
    """The oracle's fp32 blend (backends.py:461-465) for given rows."""
    adj = (1 - eta) * s32[rows] + eta * dewi32[rows]
    if pref != 0:
        adj += pref * ent32[rows]
    return adj.astype(np.float32)


def _decision(s64, adj64, nan_adj, ref_sc, k, eta, gap):
    """Cut value, first excluded value, the two gaps and the noise scales of one query.  Rows whose similarity is NaN sort
    as the LARGEST value (the reference's argpartition keeps them in the cut); the rank gap is taken over the candidates
    whose adjusted score is a number, among the k - z + 1 best of them (z: the NaN candidates that are returned)."""
    n = s64.shape[0]
    c = min(2 * k, n)
    s_key = np.where(np.isnan(s64), np.inf, s64)
    order = np.argsort(-s_key, kind="stable")
    v_c = s_key[order[c - 1]]
    v_c1 = s_key[order[c]] if c < n else -np.inf
    with np.errstate(invalid="ignore"):
        cut_gap = v_c - v_c1                       # NaN when the NaN rows alone fill the cut: never decisive
    cand = order[:c]
    numbers = cand[~nan_adj[cand]]
    z = min(int(np.count_nonzero(nan_adj[cand])), k)
    top = np.sort(adj64[numbers])[::-1][: min(k - z + 1, numbers.shape[0])]
    with np.errstate(invalid="ignore"):
        rank_gap = np.inf if top.shape[0] < 2 else float(np.min(top[:-1] - top[1:]))
    # Noise scales with the magnitude of what is compared: the similarity cut with |similarity at the cut| (l2 scores are
    # -||e - q||^2, hundreds; at eta = 1 the ADJUSTED scores stay O(1) while the cut still happens among those hundreds —
    # found by scripts/fuzz_parity.py), the ranking with the adjusted scores (which carry w_sim times the similarity).
    sim_scale = max(1.0, float(abs(v_c))) if np.isfinite(v_c) else 1.0
    ref_num = ref_sc[~np.isnan(ref_sc)]
    scale = max(1.0, float(np.max(np.abs(ref_num))) if ref_num.size else 1.0, float(abs(np.float32(1 - eta))) * sim_scale)
    g_cut = gap * sim_scale
    g = gap * scale
    decisive = bool(cut_gap > g_cut and rank_gap > g)
    return s_key, v_c, v_c1, cut_gap, rank_gap, scale, g_cut, g, decisive


def compare_query(E, q, dewi32, ent32, k, eta, pref, space, got_ids, got_scores, exact_gaps=True, gap=GAP,
                  score_tol=SCORE_TOL, prepared=False):
    """Returns (decisive: bool, message or None).  ``prepared``: q is used as given (no normalisation).

    NaN adjusted scores (a zero-norm row of a cosine corpus, a NaN row, a NaN payload value, 0 * inf) follow the
    reference (backends.py:468-471): the rows stay in the cut and in the top-k (NaN sorts as the largest value in
    argpartition) and come LAST in the result (argsort of the negated scores).  So the NaN scores of a result must be
    its tail, the ids of the tail must be the oracle's as a set whenever every NaN candidate fits into k, and the
    numbers in front of the tail are compared with the oracle's numbers under the decisive / near-tie rules."""
    s32, s64, adj64, ref_ids, ref_sc = _reference(E, q, dewi32, ent32, k, eta, pref, space, exact_gaps, prepared)
    n = s64.shape[0]
    c = min(2 * k, n)
    got_ids = np.asarray(got_ids)
    got_scores = np.asarray(got_scores)
    if got_ids.shape != ref_ids.shape:
        return False, f"shape {got_ids.shape} != {ref_ids.shape}"
    if c <= 0 or ref_ids.size == 0:
        return True, None
    with np.errstate(invalid="ignore", over="ignore"):
        nan_adj = np.isnan(_row_scores32(s32, np.arange(n), dewi32, ent32, eta, pref))     # the reference's own NaN scores
    s_key, v_c, v_c1, cut_gap, rank_gap, scale, g_cut, g, decisive = _decision(s64, adj64, nan_adj, ref_sc, k, eta, gap)
    got_nan = np.isnan(got_scores)
    z_got = int(np.count_nonzero(got_nan))
    kk = got_scores.shape[0]
    if z_got and not got_nan[kk - z_got:].all():
        return decisive, f"NaN scores are not the tail of the result: {np.nonzero(got_nan)[0].tolist()} of {kk}"
    num_ids, num_sc = got_ids[: kk - z_got], got_scores[: kk - z_got]
    tail_ids = got_ids[kk - z_got:].astype(np.int64)
    if num_sc.size > 1 and not np.all(num_sc[:-1] >= num_sc[1:]):
        return decisive, "scores not non-increasing"
    gi = got_ids.astype(np.int64)
    if gi.min() < 0 or gi.max() >= n:
        return decisive, f"row index out of range: {gi.min()}..{gi.max()}"
    if len(set(gi.tolist())) != gi.size:
        return decisive, "duplicate rows in the result"
    # ---- the NaN tail: which rows it must and may hold
    sure_cand = s_key > v_c1 + g_cut if c < n else np.ones(n, dtype=bool)
    adm_cand = s_key >= v_c - g_cut
    sure_nan, adm_nan = np.nonzero(nan_adj & sure_cand)[0], np.nonzero(nan_adj & adm_cand)[0]
    tail = set(tail_ids.tolist())
    if not tail <= set(adm_nan.tolist()):
        return decisive, f"rows {sorted(tail - set(adm_nan.tolist()))} of the NaN tail are not NaN candidates"
    if adm_nan.shape[0] <= k:                      # every NaN candidate fits: none may be missing
        if not set(sure_nan.tolist()) <= tail:
            return decisive, f"NaN candidates {sorted(set(sure_nan.tolist()) - tail)} are missing from the tail"
    elif z_got < min(k, sure_nan.shape[0]):
        return decisive, f"{z_got} NaN scores returned, at least {min(k, sure_nan.shape[0])} candidates have one"
    ref_nan = np.isnan(ref_sc)
    z_ref = int(np.count_nonzero(ref_nan))
    if decisive:
        if z_got != z_ref or not np.array_equal(num_ids, ref_ids[: kk - z_ref]):
            return decisive, f"ids differ: got {got_ids.tolist()} want {ref_ids.tolist()} (gaps {cut_gap:.2e}, {rank_gap:.2e})"
        if tail != set(ref_ids[kk - z_ref:].tolist()):
            return decisive, f"NaN tail {sorted(tail)} != the oracle's {sorted(ref_ids[kk - z_ref:].tolist())}"
        if num_sc.size:
            err = float(np.max(np.abs(num_sc.astype(np.float64) - ref_sc[: kk - z_ref].astype(np.float64))))
            if not err <= score_tol * scale:
                return decisive, f"score error {err:.3e} > {score_tol * scale:.1e}"
        return decisive, None
    # ---- near-tie query: admissible-outcome check on the ids of the numbers
    ni = num_ids.astype(np.int64)
    if ni.size == 0:
        return decisive, None
    if nan_adj[ni].any():
        return decisive, f"rows {ni[nan_adj[ni]].tolist()} carry a number but their adjusted score is NaN"
    if np.any(s_key[ni] < v_c - g_cut):
        bad = ni[s_key[ni] < v_c - g_cut]
        return decisive, f"rows {bad.tolist()} are not among the top-{c} similarities (cut {v_c:.7f}, gap {g_cut:.1e})"
    want_sc = _row_scores32(s32, ni, dewi32, ent32, eta, pref)
    err = np.abs(num_sc.astype(np.float64) - want_sc.astype(np.float64))
    if not float(np.max(err)) <= score_tol * scale:
        return decisive, f"near-tie query: score of a returned row off by {float(np.max(err)):.3e}"
    sure = sure_cand & ~nan_adj
    sure[ni] = False
    worst = float(np.min(adj64[ni]))
    if np.any(adj64[sure] > worst + g):
        x = np.nonzero(sure)[0][int(np.argmax(adj64[sure]))]
        return decisive, (f"near-tie query: row {int(x)} (adjusted {adj64[x]:.7f}) is a sure candidate and beats the "
                          f"worst returned score {worst:.7f} by more than {g:.1e} but was left out")
    return decisive, None


def device_prepared_queries(Q, space="cosine"):
    """GPU only: the library's own prepared bf16 queries (``dewi_prepare_queries_bf16``; every bf16 kernel
    normalises with the same float64-summed norm, see csrc/common.hpp ``wave_query_norm``) as fp32 values,
    AFTER checking them against the oracle's ``bf16_round(prepare_query(q))``: every element within one bf16
    ulp, at least 99 % bit-equal.  (NumPy sums ||q||^2 in fp32, so an element on a rounding boundary may
    round the other way; feeding the oracle these queries removes that one-ulp noise from the comparison,
    which can then be made at fp32-summation tolerance.)"""
    import torch
    from dewi import _engine as eng
    qd = torch.from_numpy(np.ascontiguousarray(Q, dtype=np.float32)).cuda()
    got = eng.prepare_queries_bf16(qd, space).float().cpu().numpy()
    want = np.stack([orc.bf16_round(orc.prepare_query(q, space)) for q in np.atleast_2d(Q)])
    ulp = np.abs(want) * 2.0 ** -7 + 1e-38            # one bf16 ulp is at most 2^-7 relative
    assert np.all(np.abs(got - want) <= ulp), "a prepared query element is more than one bf16 ulp off the oracle's"
    assert np.mean(got == want) >= 0.99, float(np.mean(got == want))
    return got


def default_floor(k: int) -> float:
    return 0.8 if k <= 10 else 0.25


def check_batch(E, Q, dewi32, ent32, k, eta, pref, space, ids, scores, min_decisive_frac=None, **kw):
    """Every query must pass ``compare_query``; at least ``min_decisive_frac`` of them (default by k, see
    the module docstring; never zero) must have been decisive, i.e. compared id for id.  Returns the
    decisive count."""
    floor = default_floor(k) if min_decisive_frac is None else float(min_decisive_frac)
    assert floor > 0.0, "a parity case must assert some decisive id comparisons"
    n_dec = 0
    for j in range(Q.shape[0]):
        decisive, msg = compare_query(E, Q[j], dewi32, ent32, k, eta, pref, space, ids[j], scores[j], **kw)
        assert msg is None, f"query {j}: {msg}"
        n_dec += 1 if decisive else 0
    need = int(np.ceil(floor * Q.shape[0]))
    assert n_dec >= need, f"only {n_dec}/{Q.shape[0]} queries were decisive (floor {need}): pick other seeds or a tighter gap"
    return n_dec


def count_decisive(E, Q, dewi32, ent32, k, eta, pref, space, exact_gaps=True, gap=GAP, prepared=False):
    """CPU-only: how many queries of a case are decisive (used to calibrate the floors)."""
    n_dec = 0
    for j in range(Q.shape[0]):
        s32, s64, adj64, ref_ids, ref_sc = _reference(E, Q[j], dewi32, ent32, k, eta, pref, space, exact_gaps, prepared)
        if ref_ids.size == 0:
            n_dec += 1
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            nan_adj = np.isnan(_row_scores32(s32, np.arange(s32.shape[0]), dewi32, ent32, eta, pref))
        n_dec += 1 if _decision(s64, adj64, nan_adj, ref_sc, k, eta, gap)[-1] else 0
    return n_dec

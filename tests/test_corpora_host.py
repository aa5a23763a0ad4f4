"""CPU checks of the adversarial corpora (tests/corpora.py) that tests/test_hip_dense_neighbourhoods.py searches on the GPU.

Whether a query is decisive (compared id for id, tests/parity.py) depends on the inputs and the oracle alone, so the floor the
GPU tests pass to ``check_batch`` (``min_decisive_frac=0.75``) is checked here as a CONDITION on the inputs: a case whose
queries were mostly near-ties would pass on admissibility checks alone.  Decisive counts measured with this file at eta 0.3,
pref 0.1, ``exact_gaps=False`` (fp32: gap 5e-7 on the unit rows; bf16: gap 1e-6 on the bf16-rounded rows and prepared
queries), over the queries ``corpora.oracle_queries`` picks:

    planted   n        dim   b    k    d_max   fp32    bf16
              66 000   256   40   10   200     32/32   32/32
              66 000   256   32   10   200     32/32   32/32
              65 600   1024  8    10   200     8/8     8/8
              66 000   128   32   10   200     32/32   32/32
              66 000   256   12   10   200     12/12   12/12      (the same unit rows searched in l2: 12/12)
              66 000   256   256  10   200     32/32   31/32
              66 000   256   8    10   200     8/8     8/8
              131 072  256   40   100  400     32/32   29/32
              131 072  256   32   100  400     31/32   30/32
    embedding 66 000   256   40   10           31/32   32/32      (eta 0, pref 0: 31/32, 31/32)
              66 000   256   40   100          32/32   26/32      (eta 0, pref 0: 7/32, 5/32 — not used on the GPU)

(OpenBLAS sums in an order of its own choosing: a borderline query may fall the other way on another machine, which is why
the assertion is the floor and not the count.)
"""
import numpy as np
import pytest

import corpora
import dewi_oracle as orc
import parity

FLOOR = 0.75


def _payload(n, seed):
    cols = orc.synth_payload_columns(n, seed=seed)
    return orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])


def _decisive(X, Q, seed, k, eta=0.3, pref=0.1, space="cosine"):
    d, e = _payload(X.shape[0], seed)
    f32 = parity.count_decisive(X, Q, d, e, k, eta, pref, space, exact_gaps=False)
    if space != "cosine":
        return f32, None
    Eb = orc.bf16_round(X)
    Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    return f32, parity.count_decisive(Eb, Qp, d, e, k, eta, pref, "cosine", gap=1e-6, prepared=True, exact_gaps=False)


@pytest.mark.parametrize("name", list(corpora.PLANTED_CASES))
def test_planted_runs_are_decisive_for_the_oracle(name):
    n, dim, b, k, d_max = corpora.PLANTED_CASES[name]
    X, Q, D, rows = corpora.planted_runs(n, dim, b, seed=dim + b, d_max=d_max)
    sel = corpora.oracle_queries(b)
    need = int(np.ceil(FLOOR * sel.size))
    f32, bf16 = _decisive(X, Q[sel], dim + b, k)
    print(f"{name}: fp32 {f32}/{sel.size}, bf16 {bf16}/{sel.size}")
    assert f32 >= need and bf16 >= need, (f32, bf16, need)
    if b == 12:          # the l2 route searches these unit rows unnormalised: scores -(2 - 2 cos)
        l2, _ = _decisive(X, Q[sel], dim + b, k, space="l2")
        print(f"{name}: l2 {l2}/{sel.size}")
        assert l2 >= need, (l2, need)


def test_planted_runs_are_what_they_say():
    n, dim, b, d_max, owners, step = 66_000, 64, 32, 200, 256, 2e-4
    X, Q, D, rows = corpora.planted_runs(n, dim, b, seed=5, d_max=d_max, step=step, owners=owners)
    X2, Q2, D2, rows2 = corpora.planted_runs(n, dim, b, seed=5, d_max=d_max, step=step, owners=owners)
    assert np.array_equal(X, X2) and np.array_equal(Q, Q2) and all(np.array_equal(a, c) for a, c in zip(rows, rows2))    # seeded
    assert D.tolist() == np.resize(np.unique(np.round(np.geomspace(1, d_max, b))), b).astype(int).tolist()
    assert D.min() == 1 and D.max() == d_max and [len(r) for r in rows] == D.tolist()
    assert np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1.0, atol=1e-6)
    raw = orc.synth_corpus(n, dim, 5)
    touched = np.flatnonzero((X != raw).any(axis=1))
    assert sorted(touched.tolist()) == sorted(np.concatenate(rows).tolist())                  # nothing else was overwritten
    for j in range(b):
        tiles = rows[j] // corpora.TILE_ROWS
        assert np.all(tiles % owners == (7 * j + 3) % owners)                                   # one owner's tiles
        base = np.flatnonzero((X == Q[j]).all(axis=1))
        assert base.size == 1 and base[0] < n // 2 and base[0] not in touched                  # the query is one untouched row
        cos = X[rows[j]].astype(np.float64) @ Q[j].astype(np.float64)
        want = 1.0 - step * (np.arange(D[j]) + 1.0)
        assert np.allclose(cos, want, rtol=0, atol=2e-7), float(np.max(np.abs(cos - want)))     # graded: 1 - step, 1 - 2 step, ...
        # ... and still distinct after both sides are rounded to bf16 (what a bf16 corpus scores; the rounding moves a
        # cosine by about as much as one step, so the ORDER may change — the oracle of a bf16 case runs on the rounded rows)
        cos_b = orc.bf16_round(X[rows[j]]).astype(np.float64) @ orc.bf16_round(Q[j]).astype(np.float64)
        assert np.unique(cos_b).size == cos_b.size and np.all(cos_b > 0.9)
        others = np.delete(np.arange(n), np.concatenate([rows[j], base]))
        assert float(np.max(X[others] @ Q[j])) < 0.9                                             # nothing else is close
    with pytest.raises(ValueError):
        corpora.planted_runs(n, dim, b, seed=5, d_max=32 * (n // 32 // owners) + 1, owners=owners)   # a run must fit its owner
    with pytest.raises(ValueError):
        corpora.planted_runs(n, dim, 300, seed=5, d_max=100, owners=owners)                          # one first tile per run


@pytest.mark.parametrize("k", [10, 100])
def test_embedding_like_is_decisive_for_the_oracle(k):
    n, dim, nq, seed = corpora.EMBEDDING_CASE
    X, Q, labels, q_rows = corpora.embedding_like(n, dim, seed, n_queries=nq)
    sel = corpora.oracle_queries(nq)
    need = int(np.ceil(FLOOR * sel.size))
    f32, bf16 = _decisive(X, Q[sel], seed, k)
    print(f"embedding-like k={k}: fp32 {f32}/{sel.size}, bf16 {bf16}/{sel.size}")
    assert f32 >= need and bf16 >= need, (f32, bf16, need)
    if k == 10:          # the exact-row check of the GPU test runs at eta 0, pref 0
        f32, bf16 = _decisive(X, Q[sel], seed, k, eta=0.0, pref=0.0)
        print(f"embedding-like k={k}, eta 0: fp32 {f32}/{sel.size}, bf16 {bf16}/{sel.size}")
        assert f32 >= need and bf16 >= need, (f32, bf16, need)


def test_embedding_like_is_what_it_says():
    n, dim, nq, seed = 20_000, 256, 12, 3
    X, Q, labels, q_rows = corpora.embedding_like(n, dim, seed, n_queries=nq)
    X2, Q2, _, _ = corpora.embedding_like(n, dim, seed, n_queries=nq)
    assert np.array_equal(X, X2) and np.array_equal(Q, Q2)
    assert np.all(np.diff(labels) >= 0)                                   # one source after another
    sizes = np.bincount(labels, minlength=48)
    assert sizes.max() > 4 * n // 48                                      # skewed: the largest source is several times the mean
    assert np.allclose(np.linalg.norm(X.astype(np.float64), axis=1), 1.0, atol=1e-6)
    S = X[::7].astype(np.float64) @ X[::11].astype(np.float64).T
    assert 0.35 < S.min() and np.median(S) > 0.55                         # every pair of rows is similar: no score near 0
    assert np.array_equal(Q[:4], X[q_rows[:4]])                           # exact corpus rows
    own = np.einsum("qd,qd->q", Q.astype(np.float64), X[q_rows].astype(np.float64))
    assert np.all(own[4:] > 0.99) and np.all(own[4:] < 1.0 - 1e-4)        # the others: near their row, not on it

"""Seeded corpora arranged AGAINST the samplers of the batched matrix-core searches (helper module, no tests).

Every other kNN parity test draws corpus and queries i.i.d. Gaussian (``orc.synth_corpus``): all cosines ~N(0, 1/dim), a
query's survivors spread evenly over the workgroups, nothing refused.  The two generators here make the other regimes:

``planted_runs``     runs of graded near-copies of a query's base row, every run inside the tiles of ONE workgroup of the
                     filter pass (tiles are dealt round-robin: tile t belongs to workgroup t mod n_blocks), with run lengths
                     that sweep from 1 to ``d_max`` across the batch — so that the survivor segment of (workgroup, query)
                     is under, at and over its capacity for different queries of one call.
``embedding_like``   anisotropic, clustered rows in source order: all pairwise cosines in about 0.4 .. 1.0, scores crowded
                     into a narrow band below 1.

Both return unit-norm fp32 rows (what a cosine corpus stores), so the CPU checks can use them as the oracle's matrix.
"""
import numpy as np

import dewi_oracle as orc

TILE_ROWS = 32          # rows per tile of every matrix-core pass (csrc/knn_mfma_bf16.hip kTileRows, knn_mfma_f32.hip kF32TileRows)


#: the planted-run inputs of tests/test_hip_dense_neighbourhoods.py: (n, dim, b, k, d_max); the seed is dim + b.  A run must fit
#: its owner's rows, d_max <= 32 floor(n_tiles / owners) — 256 at 66 000 rows and 256 owners, which is why k = 100 (whose
#: capacities need longer runs) has 131 072 rows.  tests/test_corpora_host.py counts their decisive queries on the CPU.
PLANTED_CASES = {
    "n66000-d256-b40": (66_000, 256, 40, 10, 200),
    "n66000-d256-b32": (66_000, 256, 32, 10, 200),
    "n65600-d1024-b8": (65_600, 1024, 8, 10, 200),
    "n66000-d128-b32": (66_000, 128, 32, 10, 200),
    "n66000-d256-b12": (66_000, 256, 12, 10, 200),
    "n66000-d256-b256": (66_000, 256, 256, 10, 200),
    "n66000-d256-b8": (66_000, 256, 8, 10, 200),
    "n131072-d256-b40-k100": (131_072, 256, 40, 100, 400),
    "n131072-d256-b32-k100": (131_072, 256, 32, 100, 400),
}
#: the embedding-like input of the same tests: (n, dim, n_queries, seed)
EMBEDDING_CASE = (66_000, 256, 40, 11)


def oracle_queries(b, n_max=32):
    """The at most ``n_max`` queries of a batch of ``b`` that the oracle checks: all of them, or ``n_max`` spread evenly
    over the batch (and so over the sweep of run lengths), first and last included."""
    return np.arange(b) if b <= n_max else np.unique(np.round(np.linspace(0, b - 1, n_max)).astype(np.int64))


def _unit(x):
    x = np.asarray(x, dtype=np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def run_lengths(b, d_max):
    """D_j for the queries of a batch of ``b``: ``unique(round(geomspace(1, d_max, b)))`` recycled to length b."""
    lengths = np.unique(np.round(np.geomspace(1, d_max, b)).astype(np.int64))
    return np.resize(lengths, b)


def planted_runs(n, dim, b, seed, d_max, step=2e-4, owners=256):
    """``(X fp32 [n, dim], Q fp32 [b, dim], D int64 [b], rows)``: ``orc.synth_corpus(n, dim, seed)`` with, for every query j,
    a run of ``D[j]`` graded near-copies of its base row ``r_j`` written over the rows ``rows[j]`` (int64 [D[j]], in the order
    of the grading).  Near-copy i is ``unit(c_i e + sqrt(1 - c_i^2) v_i)`` with e = row r_j, ``c_i = 1 - step (i + 1)`` and v_i
    a random unit vector orthogonal to e: the true cosines of query j (= e itself, self-match exactly 1) to its run are
    1 - step, 1 - 2 step, ...  Run j fills the tiles ``t0_j + i owners`` (i = 0, 1, ...), ``t0_j = (7 j + 3) mod owners``, 32
    rows each: with ``owners`` = the number of workgroups of the filter pass, ``min(n_tiles, compute units)``, all of them
    tiles of workgroup t0_j.  A run must fit the whole tiles every owner has: ``d_max <= 32 floor(n_tiles / owners)``.
    Base rows come from the first half of the corpus, outside every planted tile, distinct."""
    n_tiles = (n + TILE_ROWS - 1) // TILE_ROWS
    owners = int(min(owners, n_tiles))
    per_owner = (n // TILE_ROWS) // owners                       # whole tiles every owner surely has
    if d_max > TILE_ROWS * per_owner:
        raise ValueError(f"d_max = {d_max} exceeds the {TILE_ROWS * per_owner} rows one of {owners} owners has in {n} rows")
    t0 = (7 * np.arange(b) + 3) % owners
    if np.unique(t0).size != b:
        raise ValueError(f"{b} runs do not get distinct first tiles among {owners} owners")
    X = orc.synth_corpus(n, dim, seed)
    D = run_lengths(b, d_max)
    rng = np.random.default_rng(seed)
    rows = []
    planted = np.zeros(n, dtype=bool)
    for j in range(b):
        i = np.arange(int(D[j]), dtype=np.int64)
        r = TILE_ROWS * (t0[j] + (i // TILE_ROWS) * owners) + i % TILE_ROWS
        assert r.max() < n
        rows.append(r)
        planted[(r // TILE_ROWS * TILE_ROWS)[:, None] + np.arange(TILE_ROWS)[None, :]] = True     # the whole tiles
    free = np.flatnonzero(~planted[: n // 2])
    base = rng.choice(free, size=b, replace=False)
    for j in range(b):
        e = _unit(X[base[j]])
        g = rng.standard_normal((int(D[j]), dim))
        v = _unit(g - (g @ e)[:, None] * e[None, :])
        c = 1.0 - step * (np.arange(int(D[j]), dtype=np.float64) + 1.0)
        X[rows[j]] = _unit(c[:, None] * e[None, :] + np.sqrt(1.0 - c * c)[:, None] * v).astype(np.float32)
    Q = X[base].copy()
    return X, Q, D, rows


def embedding_like(n, dim, seed, n_centres=48, noise=0.6, shift=1.5, n_queries=32, query_noise=0.1, chunk=65536):
    """``(X fp32 [n, dim], Q fp32 [n_queries, dim], labels int64 [n], query_rows int64 [n_queries])``.  Cluster sizes are
    skewed (``Dirichlet(0.3)``), rows sorted by cluster (one source after another) and equal to
    ``unit(centre[label] + noise randn + shift sqrt(dim) u)`` for Gaussian centres and one fixed unit vector u: all pairwise
    cosines lie in about 0.4 .. 1.0 (different clusters ~ shift^2 / (shift^2 + 1 + noise^2), the same cluster
    ~ (shift^2 + 1) / (shift^2 + 1 + noise^2)).  Queries are ``unit(row + query_noise randn / sqrt(dim))`` of random rows
    ``query_rows`` (cosine to the own row ~ 1 - query_noise^2 / 2); the first four are the rows themselves."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_centres, dim))
    u = _unit(rng.standard_normal(dim))
    labels = np.sort(rng.choice(n_centres, size=n, p=rng.dirichlet(np.full(n_centres, 0.3))))
    X = np.empty((n, dim), dtype=np.float32)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        blk = centres[labels[s:e]] + noise * rng.standard_normal((e - s, dim)) + (shift * np.sqrt(dim)) * u[None, :]
        X[s:e] = _unit(blk).astype(np.float32)
    query_rows = rng.choice(n, size=n_queries, replace=False)
    Q = _unit(X[query_rows].astype(np.float64) + (query_noise / np.sqrt(dim)) * rng.standard_normal((n_queries, dim))).astype(np.float32)
    Q[:4] = X[query_rows[:4]]
    return X, Q, labels, query_rows

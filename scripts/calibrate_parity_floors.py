#!/usr/bin/env python3
"""CPU-only calibration of the decisive-query floors the GPU parity tests assert (tests/parity.py).

Whether a query is "decisive" depends on the inputs and the oracle alone (float64 gaps), not on the GPU
result, so the share of decisive queries of every seeded test case can be counted here, without a GPU:

    python3 scripts/calibrate_parity_floors.py

The floors in tests/test_hip_search.py, test_hip_bf16.py and test_hip_mfma.py sit a little below these
counts (stored rows come from the device's normalisation kernel and can differ from the oracle's in the
last fp32 bit, which may move a borderline query across the gap).
"""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "oracle"))
sys.path.insert(0, str(REPO / "tests"))
import numpy as np  # noqa: E402

import dewi_oracle as orc  # noqa: E402
import parity  # noqa: E402


def soa(cols):
    return orc.payload_soa(cols["dewi"], cols["ht_mean"], cols["hi_mean"])


print("== dimension sweep")
for dim in [8, 10, 16, 100, 128, 256, 260, 512, 768, 1024, 1536, 2048]:
    n = 3001 if dim <= 1024 else 1500
    raw = orc.synth_corpus(n, dim, seed=dim); cols = orc.synth_payload_columns(n, seed=dim)
    Q = orc.synth_queries(5, dim, seed=dim + 1); E = orc.build_matrix(raw); d,e = soa(cols)
    print(dim, [parity.count_decisive(E,Q,d,e,k,eta,pref,"cosine") for k,eta,pref in ((1, 0.3, 0.0), (10, 0.3, 0.0), (10, 0.7, -0.5), (100, 0.25, 0.3), (150, 0.5, 0.0))])
print("== l2")
for dim in [16,100,768]:
    rs = np.random.RandomState(dim); raw = (rs.randn(2000, dim) * 0.5).astype(np.float32)
    cols = orc.synth_payload_columns(2000, seed=3); Q = (rs.randn(5, dim) * 0.5).astype(np.float32); d,e=soa(cols)
    print(dim, parity.count_decisive(raw,Q,d,e,10,0.3,0.0,"l2"))
print("== eight queries")
for space in ["cosine","l2"]:
  for dim in [256,768,1536]:
    rs = np.random.RandomState(dim); scale = 0.5 if space == "l2" else 1.0
    raw = (rs.randn(3001, dim) * scale).astype(np.float32); cols = orc.synth_payload_columns(3001, seed=dim)
    Q = (rs.randn(21, dim) * scale).astype(np.float32); d,e=soa(cols)
    E = orc.build_matrix(raw) if space=="cosine" else raw
    print(space, dim, parity.count_decisive(E,Q,d,e,10,0.3,0.1,space), "/21")
def rnd_cases(n_cases, seed):
    rs = np.random.RandomState(seed)
    dims = [1, 3, 7, 8, 24, 33, 64, 96, 100, 128, 129, 200, 256, 384, 512, 640, 768, 1000]
    out = []
    for _ in range(n_cases):
        n = int(rs.choice([1, 2, 3, 17, 64, 255, 256, 257, 1000, 2049, 4000]))
        dim = int(rs.choice(dims)); b = int(rs.randint(1, 10)); k = int(rs.randint(1, min(n, 300) + 1))
        eta = float(rs.choice([0.0, 0.3, 0.5, 1.0, rs.rand()])); pref = float(rs.choice([0.0, -1.0, 0.5, rs.uniform(-1, 1)]))
        space = str(rs.choice(["cosine", "cosine", "l2"]))
        out.append((n, dim, b, k, eta, pref, space))
    return out
print("== fp32 random")
tot=dec=0
for case in rnd_cases(36, 20261004):
    n, dim, b, k, eta, pref, space = case
    rs = np.random.RandomState(n * 31 + dim)
    raw = (rs.randn(n, dim) * (0.5 if space == "l2" else 1.0)).astype(np.float32)
    cols = orc.synth_payload_columns(n, seed=dim)
    Q = (rs.randn(b, dim) * (0.5 if space == "l2" else 1.0)).astype(np.float32)
    with np.errstate(all='ignore'):
        E = orc.build_matrix(raw) if space=="cosine" else raw
    d,e=soa(cols)
    nd = parity.count_decisive(E,Q,d,e,k,eta,pref,space)
    tot+=b; dec+=nd
    print(case[:4], case[6], f"eta={eta:.2f} pref={pref:.2f}", nd, "/", b)
print(dec, tot)
def rnd_bf16(n_cases, seed):
    rs = np.random.RandomState(seed); out = []
    for _ in range(n_cases):
        n = int(rs.choice([1, 2, 3, 5, 64, 255, 257, 1001, 3000])); dim = int(rs.choice([8, 9, 40, 100, 128, 256, 300, 512, 768]))
        b = int(rs.randint(1, 10)); k = int(rs.randint(1, min(n, 120) + 1))
        out.append((n, dim, b, k, float(rs.choice([0.0, 0.3, 1.0])), float(rs.choice([0.0, 0.4, -1.0]))))
    return out
print("== bf16 random, gap 2e-5 / 4e-6")
tot=dec=dec2=0
for case in rnd_bf16(24, 4102026):
    n, dim, b, k, eta, pref = case
    raw = orc.synth_corpus(n, dim, seed=n * 7 + dim); cols = orc.synth_payload_columns(n, seed=n * 7 + dim)
    Eb = orc.bf16_round(orc.build_matrix(raw)); d,e=soa(cols)
    Q = orc.synth_queries(b, dim, seed=dim + b); Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    nd = parity.count_decisive(Eb,Qp,d,e,k,eta,pref,"cosine",gap=2e-5,prepared=True)
    nd2 = parity.count_decisive(Eb,Qp,d,e,k,eta,pref,"cosine",gap=4e-6,prepared=True)
    tot+=b; dec+=nd; dec2+=nd2
    print(case, nd, nd2, "/", b)
print(dec, dec2, tot)
print("== bf16 fixed")
for dim,n in [(768, 4001), (768, 4000), (512, 3000), (256, 2501), (1024, 1501), (136, 2000), (100, 2000), (1280, 900)]:
    raw = orc.synth_corpus(n, dim, seed=dim+n); cols = orc.synth_payload_columns(n, seed=dim+n)
    Eb = orc.bf16_round(orc.build_matrix(raw)); d,e=soa(cols)
    Q = orc.synth_queries(5, dim, seed=dim); Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    print(dim,n,[parity.count_decisive(Eb,Qp,d,e,k,eta,pref,"cosine",gap=2e-5,prepared=True) for k,eta,pref in ((10, 0.3, 0.0), (1, 0.5, 0.0), (100, 0.25, 0.3), (150, 0.5, 0.0))])
G = 1e-6
def rnd_bf16(n_cases, seed):
    rs = np.random.RandomState(seed); out = []
    for _ in range(n_cases):
        n = int(rs.choice([1, 2, 3, 5, 64, 255, 257, 1001, 3000])); dim = int(rs.choice([8, 9, 40, 100, 128, 256, 300, 512, 768]))
        b = int(rs.randint(1, 10)); k = int(rs.randint(1, min(n, 120) + 1))
        out.append((n, dim, b, k, float(rs.choice([0.0, 0.3, 1.0])), float(rs.choice([0.0, 0.4, -1.0]))))
    return out
for case in rnd_bf16(24, 4102026):
    n, dim, b, k, eta, pref = case
    raw = orc.synth_corpus(n, dim, seed=n * 7 + dim); cols = orc.synth_payload_columns(n, seed=n * 7 + dim)
    Eb = orc.bf16_round(orc.build_matrix(raw)); d,e=soa(cols)
    Q = orc.synth_queries(b, dim, seed=dim + b); Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    nd = parity.count_decisive(Eb,Qp,d,e,k,eta,pref,"cosine",gap=G,prepared=True)
    if nd<b: print(case, nd, "/", b)
print("== bf16 fixed")
for dim,n in [(768, 4001), (768, 4000), (512, 3000), (256, 2501), (1024, 1501), (136, 2000), (100, 2000), (1280, 900)]:
    raw = orc.synth_corpus(n, dim, seed=dim+n); cols = orc.synth_payload_columns(n, seed=dim+n)
    Eb = orc.bf16_round(orc.build_matrix(raw)); d,e=soa(cols)
    Q = orc.synth_queries(5, dim, seed=dim); Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    print(dim,n,[parity.count_decisive(Eb,Qp,d,e,k,eta,pref,"cosine",gap=G,prepared=True) for k,eta,pref in ((10, 0.3, 0.0), (1, 0.5, 0.0), (100, 0.25, 0.3), (150, 0.5, 0.0))])
print("== mfma cases")
for dim,n,b,k in [(768, 70_001, 256, 100), (768, 66_000, 40, 10), (512, 80_000, 300, 10), (256, 70_000, 17, 100), (128, 131_072, 64, 10)]:
    raw = orc.synth_corpus(n, dim, seed=dim+b); cols = orc.synth_payload_columns(n, seed=dim+b)
    Eb = orc.bf16_round(raw); d,e=soa(cols)
    Q = orc.synth_queries(b, dim, seed=b)[:32]; Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    print(dim,n,b,k, parity.count_decisive(Eb,Qp,d,e,k,0.3,0.1,"cosine",gap=G,prepared=True,exact_gaps=False), "/", len(Q))
print("== dense neighbourhoods (tests/corpora.py): fp32 / bf16 decisive among the queries the oracle checks; the GPU tests' floor is 0.75")
import corpora  # noqa: E402
def both(X, Q, seed, k, eta=0.3, pref=0.1):
    d, e = soa(orc.synth_payload_columns(X.shape[0], seed=seed))
    Eb = orc.bf16_round(X); Qp = np.stack([orc.bf16_round(orc.prepare_query(q)) for q in Q])
    return (parity.count_decisive(X, Q, d, e, k, eta, pref, "cosine", exact_gaps=False),
            parity.count_decisive(Eb, Qp, d, e, k, eta, pref, "cosine", gap=G, prepared=True, exact_gaps=False))
for name, (n, dim, b, k, d_max) in corpora.PLANTED_CASES.items():
    X, Q, D, rows = corpora.planted_runs(n, dim, b, seed=dim + b, d_max=d_max)
    sel = corpora.oracle_queries(b)
    print("planted", name, "k", k, both(X, Q[sel], dim + b, k), "/", sel.size)
n, dim, nq, seed = corpora.EMBEDDING_CASE
X, Q, _, _ = corpora.embedding_like(n, dim, seed, n_queries=nq)
sel = corpora.oracle_queries(nq)
for k, eta, pref in ((10, 0.3, 0.1), (10, 0.0, 0.0), (100, 0.3, 0.1), (100, 0.0, 0.0)):
    print("embedding-like k", k, "eta", eta, "pref", pref, both(X, Q[sel], seed, k, eta, pref), "/", sel.size)
print("== non-finite order (tests/test_hip_nonfinite_order.py, and the NaN-row tests of test_hip_search / test_hip_mfma_f32)")
import test_hip_nonfinite_order as nf  # noqa: E402
def build(raw, space):
    with np.errstate(all="ignore"):
        if space != "cosine":
            return raw
        return (raw / np.linalg.norm(raw, axis=1, keepdims=True)).astype(np.float32)   # rows as orc.build_matrix, vectorised
def bf16_inputs(E, Q, space="cosine"):
    return orc.bf16_round(E), np.stack([orc.bf16_round(orc.prepare_query(q, space)) for q in Q])
for space in ("cosine", "l2"):
    for dim in (256, 100, 10):
        out = []
        for k in (5, 40, 150):
            raw, cols, Q, bad = nf.corpus(300, dim, space, seed=dim + k, n_bad=3 if k == 5 else 7)
            d, e = soa(cols)
            out.append(parity.count_decisive(build(raw, space), Q, d, e, k, nf.ETA, nf.PREF, space))
        print("one query f32", space, dim, "k 5/40/150:", out, "/ 4")
raw, cols, Q, bad = nf.corpus(3000, 64, "cosine", seed=71, n_bad=9, b=2); d, e = soa(cols)
print("k 1025:", parity.count_decisive(build(raw, "cosine"), Q, d, e, 1025, nf.ETA, 0.1, "cosine"), "/ 2")
for dim in (256, 100):
    raw, cols, Q, bad = nf.corpus(300, dim, "cosine", seed=dim + 3, n_bad=4); d, e = soa(cols)
    Eb, Qp = bf16_inputs(build(raw, "cosine"), Q)
    print("one query bf16", dim, parity.count_decisive(Eb, Qp, d, e, 10, nf.ETA, nf.PREF, "cosine", gap=G, prepared=True, exact_gaps=False), "/ 4")
for route in nf.BATCH_ROUTES:
    raw, cols, Q, bad, elem, space, kernel = nf.batch_case(route); d, e = soa(cols)
    sel = np.linspace(0, Q.shape[0] - 1, nf.BATCH_CHECKED).astype(int)
    E = build(raw, space)
    if elem == "bf16":
        Eb, Qp = bf16_inputs(E, Q[sel], space)
        nd = parity.count_decisive(Eb, Qp, d, e, nf.BATCH_K, nf.ETA, 0.1, space, gap=G, prepared=True, exact_gaps=False)
    else:
        nd = parity.count_decisive(E, Q[sel], d, e, nf.BATCH_K, nf.ETA, 0.1, space, exact_gaps=False)
    print("batch", route, nd, "/", sel.size)
raw, cols, Q, bad = nf.corpus(3000, 96, "cosine", seed=96, n_bad=5, b=6); d, e = soa(cols); E = build(raw, "cosine")
masks = np.random.RandomState(4).rand(6, 3000) < 0.4; masks[:, bad[:3]] = True; masks[:, bad[3:]] = False; masks[1, bad[3]] = True
print("lists:", sum(parity.count_decisive(E[masks[j]], Q[j:j + 1], d[masks[j]], e[masks[j]], 10, nf.ETA, nf.PREF, "cosine") for j in range(6)), "/ 6 (each compared twice)")
for n, dim, k in ((3000, 96, 10), (6000, 64, 200)):
    raw, cols, Q, bad = nf.corpus(n, dim, "cosine", seed=dim + k, n_bad=7, b=4); d, e = soa(cols)
    print("shards", n, dim, k, parity.count_decisive(build(raw, "cosine"), Q, d, e, k, nf.ETA, nf.PREF, "cosine"), "/ 4")
raw, cols, Q, rows = nf.payload_case(300, 100, 4, seed=8); d, e = soa(cols)
print("NaN dewi, one query:", parity.count_decisive(build(raw, "cosine"), Q, d, e, 5, nf.ETA, nf.PREF, "cosine"), "/ 4")
raw, cols, Q, rows = nf.payload_case(66_000, 128, 32, seed=9); d, e = soa(cols)
sel = np.linspace(0, 31, nf.BATCH_CHECKED).astype(int)
print("NaN dewi, batch:", parity.count_decisive(build(raw, "cosine"), Q[sel], d, e, 10, nf.ETA, nf.PREF, "cosine", exact_gaps=False), "/", sel.size)
# tests/test_hip_search.py::test_nan_rows_rank_last_like_numpy
rs = np.random.RandomState(6); raw = rs.randn(300, 256).astype(np.float32); raw[17] = 0
cols = orc.synth_payload_columns(300, seed=6); d, e = soa(cols); q = rs.randn(256).astype(np.float32)
print("test_nan_rows_rank_last_like_numpy:", parity.count_decisive(build(raw, "cosine"), q[None, :], d, e, 5, 0.3, 0.0, "cosine"), "/ 1",
      "gaps", orc.decision_gaps(np.delete(build(raw, "cosine"), 17, axis=0), q, np.delete(d, 17), np.delete(e, 17), 4, 0.3))
# tests/test_hip_mfma_f32.py::test_partial_chunk_keeps_a_nan_row_out_of_its_neighbours (k = 5, eta = 0, 16 queries, 3 NaN rows)
for dim in (384, 96, 800, 200, 1000, 300, 100, 260, 1284):
    n, k, b = 70_000, 5, 16
    raw = orc.synth_corpus(n, dim, seed=dim)
    for i in (1000, 31 + 32 * 7, n - 1):
        raw[i] = 0.0
    cols = orc.synth_payload_columns(n, seed=dim); d, e = soa(cols)
    Q = orc.synth_queries(b, dim, seed=3); Q[0], Q[1], Q[2] = raw[999], raw[30 + 32 * 7], raw[n - 2]
    E = build(raw, "cosine")
    Eb, Qp = bf16_inputs(E, Q)
    print("partial chunk", dim, "f32", parity.count_decisive(E, Q, d, e, k, 0.0, 0.0, "cosine", exact_gaps=False),
          "bf16", parity.count_decisive(Eb, Qp, d, e, k, 0.0, 0.0, "cosine", gap=G, prepared=True, exact_gaps=False), "/", b)
# tests/test_hip_mfma_f32.py::test_mfma_depth_pass_edge_rows (k = 10, eta = 0, 16 queries)
for space, bf16 in (("cosine", False), ("l2", False), ("l2", True)):
    n, dim, b, k = 70_003, 512, 16, 10
    rng = np.random.default_rng(11)
    raw = orc.synth_corpus(n, dim, seed=11) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    raw[40_000] = np.nan if space == "l2" else 0.0
    raw[123] = 0.0 if space == "l2" else raw[123]
    Q = orc.synth_queries(b, dim, seed=12) * np.float32(0.05); Q[:4] = raw[[5, 69_999, 70_002, 31_000]]
    cols = orc.synth_payload_columns(n, seed=11); d, e = soa(cols)
    E = build(raw, space)
    if bf16:
        Eb, Qp = bf16_inputs(E, Q, space)
        nd = parity.count_decisive(Eb, Qp, d, e, k, 0.0, 0.0, space, gap=G, prepared=True, exact_gaps=False)
    else:
        nd = parity.count_decisive(E, Q, d, e, k, 0.0, 0.0, space, exact_gaps=False)
    print("edge rows", space, "bf16" if bf16 else "f32", nd, "/", b)

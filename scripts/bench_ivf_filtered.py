"""The IVF probe under a user filter (``IVFIndex.search_probe_filtered_device``) at 1 M x 768, nlist 1024, against what a
filtered search on an ``IVFIndex`` costs today and against the unfiltered probe, in one process, the routes alternating round
by round (medians of ``rounds`` rounds of ``iters`` back-to-back calls between device events, with the min-max spread of the
rounds).  The corpus is ``tests/corpora.embedding_like``; the allow-lists are random rows.

Per nprobe in --nprobe, allow-list in --fractions and batch in (1, 32), k = 10:

    probe_filtered_fp32   search_probe_filtered_device(approx=False)                  [whole call, its read-backs included]
    probe_filtered_int8   search_probe_filtered_device(approx=True)                   [whole call]
    exact_filtered        DeviceCorpus.search_device(filter=): what IVFIndex.search(filter=) runs today      [baseline a]
    probe_unfiltered      IVFIndex.search_device(nprobe=, approx=False): the same probe without the filter   [baseline b]
    prepare_filtered      dewi_ivf_probe_prepare_filtered alone                       [host clock, the read-back included]
    prepare_unfiltered    dewi_ivf_probe_prepare alone                                [host clock, the read-back included]

and recall@k of the fp32 route against the exact filtered search of the same run, with ``widen`` off and on (with the mean
``nprobe`` the widened queries ended at).

    python scripts/bench_ivf_filtered.py [--n 1048576] [--dim 768] [--nlist 1024] [--iters 30] [--rounds 5] [--json out.jsonl]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "oracle"))      # (tests/corpora.py builds its corpora on the oracle's generators)


def _events(torch, fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def _alternate(torch, routes, rounds, iters, warmup):
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    r = {key: [] for key in routes}
    for _ in range(rounds):
        for key, fn in routes.items():
            r[key].append(_events(torch, fn, iters))
    return {key: (statistics.median(v), min(v), max(v)) for key, v in r.items()}


def _host_clock(torch, fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t) * 1e3 / iters


def _recall(np, got, want, k):
    per = []
    for j in range(got.shape[0]):
        w = set(want[j][want[j] >= 0].tolist())
        per.append(len(set(got[j].tolist()) & w) / max(len(w), 1))
    return round(float(np.mean(per)), 4), round(float(np.min(per)), 4)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--fractions", default="0.01,0.1,0.5,1.0")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", default="1,4,16,64")
    ap.add_argument("--train-iters", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import numpy as np
    import torch
    from corpora import embedding_like
    from dewi.ivf import IVFIndex

    n, d, k, eta = a.n, a.dim, a.k, a.eta
    X, Q, _, _ = embedding_like(n, d, 3)
    out = open(a.json, "w") if a.json else None
    print(f"corpus {n} x {d} fp32 embedding_like, nlist {a.nlist}, k {k}, eta {eta}, {a.rounds} rounds of {a.iters} calls")
    rs = np.random.RandomState(0)
    cols = {"dewi": rs.rand(n), "ht_mean": rs.rand(n), "hi_mean": rs.rand(n)}
    idx = IVFIndex(d, "cosine", nlist=a.nlist, train_iters=a.train_iters, int8_codes=True)
    idx.add_batch_columns([f"doc_{i:08d}" for i in range(n)], X, cols)
    t = time.perf_counter()
    idx.build()
    torch.cuda.synchronize()
    sizes = idx.cell_sizes
    print(f"build {time.perf_counter() - t:.2f} s; cells of {int(sizes.min())}-{int(sizes.max())} rows (median {int(np.median(sizes))})")
    corpus, st = idx._corpus, idx._ivf
    Qd = torch.from_numpy(Q[:32]).cuda()

    for frac in [float(x) for x in a.fractions.split(",")]:
        mask = np.ones(n, bool) if frac >= 1.0 else rs.rand(n) < frac
        f = corpus.make_filter(mask)
        allow = f.byte_mask()
        exact_ids = corpus.search_device(Qd, k, 0.0, 0.0, filter=f)[0].cpu().numpy()
        for npb in [int(x) for x in a.nprobe.split(",")]:
            plain = idx.search_probe_filtered_device(Qd, k, 0.0, 0.0, filter=f, nprobe=npb)[0].cpu().numpy()
            wide = idx.search_probe_filtered_device(Qd, k, 0.0, 0.0, filter=f, nprobe=npb, widen=True, return_nprobe=True)
            i8 = idx.search_probe_filtered_device(Qd, k, 0.0, 0.0, filter=f, nprobe=npb, approx=True)[0].cpu().numpy()
            rec_plain, rec_wide = _recall(np, plain, exact_ids, k), _recall(np, wide[0].cpu().numpy(), exact_ids, k)
            rec_i8 = _recall(np, i8, exact_ids, k)
            mean_npb = float(wide[2].double().mean().item())
            print(f"\nallow-list {f.n_allowed} rows ({frac:.0%}), nprobe {npb}: recall@{k} vs the exact filtered search (mean, min) "
                  f"fp32 {rec_plain}, int8 {rec_i8}, widened {rec_wide} at a mean nprobe of {mean_npb:.1f}")
            for b in (1, 32):
                q = Qd[:b].contiguous()
                ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
                sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
                routes = {
                    "probe_filtered_fp32": lambda: idx.search_probe_filtered_device(q, k, eta, 0.0, filter=f, nprobe=npb),
                    "probe_filtered_int8": lambda: idx.search_probe_filtered_device(q, k, eta, 0.0, filter=f, nprobe=npb, approx=True),
                    "exact_filtered": lambda: corpus.search_device(q, k, eta, 0.0, ids, sc, filter=f),
                    "probe_unfiltered": lambda: idx.search_device(q, k, eta, 0.0, nprobe=npb, approx=False),
                }
                res = _alternate(torch, routes, a.rounds, a.iters, a.warmup)
                pids = st.coarse.search_device(q, npb, 0.0, 0.0, candidates=npb)[0]
                prep_f = _host_clock(torch, lambda: idx._prepare_probe_filtered(pids, b, npb, allow, 0), a.iters)
                prep_u = _host_clock(torch, lambda: idx._prepare_probe(pids, b, npb), a.iters)
                n_union, n_allowed, _ = idx._prepare_probe_filtered(pids, b, npb, allow, 0)
                rec = {"case": "ivf_filtered", "fraction": frac, "n_allowed": f.n_allowed, "nprobe": npb, "batch": b, "k": k, "n": n,
                       "dim": d, "nlist": a.nlist, "iters": a.iters, "rounds": a.rounds, "rows_listed_mean": round(float(np.mean(n_allowed)), 1),
                       "queries_below_cut": int(sum(1 for x in n_allowed if x < 2 * k)), "prepare_filtered_ms": round(prep_f, 5),
                       "prepare_unfiltered_ms": round(prep_u, 5), "recall_fp32_mean_min": rec_plain, "recall_int8_mean_min": rec_i8,
                       "recall_widened_mean_min": rec_wide, "widened_mean_nprobe": round(mean_npb, 2)}
                print(f"  batch {b}: {rec['rows_listed_mean']:.0f} rows listed per query, {rec['queries_below_cut']} below the cut; "
                      f"prepare {prep_f:.4f} ms filtered, {prep_u:.4f} ms unfiltered [host clock]")
                for key, (med, lo, hi) in res.items():
                    rec[key + "_ms"], rec[key + "_spread_ms"] = round(med, 5), [round(lo, 5), round(hi, 5)]
                    print(f"    {key:<20} {med:9.4f} ms   ({lo:.4f} - {hi:.4f})")
                if out:
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()

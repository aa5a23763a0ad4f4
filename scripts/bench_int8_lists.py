"""The int8 route over allow-lists and IVF probes at 1 M x 768 against the fp32 routes of the same build, in one process, the
routes alternating round by round (medians of ``rounds`` rounds of ``iters`` back-to-back calls between device events, with
the min-max spread of the rounds).  The corpus is ``tests/corpora.embedding_like`` (clustered unit rows, 32 queries near rows
of the corpus).

  --part lists   random allow-lists of --fractions of the rows, one query and four, k = 10:
                   fp32_filtered    search_device(filter=)                              [device, whole search]
                   int8_filtered    search_approx_filtered_device (re-scored)           [device, whole search]
                   int8_unfiltered  search_approx_device, at 100 % only                 [device, whole search]
                 the scan kernels alone from the library's timing brackets, with the algorithmic bytes
                 |A| (dim + 4) + 4 |A| + nq dim 4 (fp32: |A| dim 4 + 4 |A| + nq dim 4) over that time as a share of the
                 8 TB/s HBM peak, and recall@k of the re-scored int8 answer against the exact filtered answer.
  --part ivf     IVFIndex(nlist = 1024, int8_codes=True), nprobe in --nprobe, one query and 32: approx=True against
                 approx=False on the same index, with the split of scripts/bench_ivf.py (coarse: events; prepare: wall clock,
                 the read-back included; scan + select on a prepared buffer: events) and recall@k of both against the exact
                 search of the same run.

    python scripts/bench_int8_lists.py --part lists|ivf [--n 1048576] [--dim 768] [--k 10] [--iters 50] [--rounds 5] [--json out.jsonl]
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

HBM_PEAK = 8.0e12


def _events(torch, fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def _scan_ms(torch, eng, fn, iters):
    eng.timing(1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ms, launches = eng.timing_read()
    eng.timing(0)
    return ms, launches


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


def _recall(np, got, want, k):
    per = [len(set(got[j].tolist()) & set(want[j].tolist())) / k for j in range(got.shape[0])]
    return round(float(np.mean(per)), 4), round(float(np.min(per)), 4)


def part_lists(a, np, torch, eng, X, Q, out):
    n, d, k, eta = a.n, a.dim, a.k, a.eta
    rs = np.random.RandomState(0)
    corpus = eng.DeviceCorpus.from_host(X, rs.rand(n), rs.rand(n), rs.rand(n), "cosine").enable_int8_shadow()
    Qd = torch.from_numpy(Q).cuda()
    for frac in [float(x) for x in a.fractions.split(",")]:
        mask = np.ones(n, bool) if frac >= 1.0 else rs.rand(n) < frac
        f = corpus.make_filter(mask)
        n_a = f.n_allowed
        exact = corpus.search_device(Qd, k, 0.0, 0.0, filter=f)[0].cpu().numpy()
        approx = corpus.search_approx_filtered_device(Qd, k, 0.0, 0.0, f)[0].cpu().numpy()
        recall = _recall(np, approx, exact, k)
        print(f"\nlist of {n_a} rows ({frac:.0%}): recall@{k} of the re-scored int8 answer vs the exact filtered answer "
              f"(mean, min over {Qd.shape[0]} queries): {recall}")
        for b in (1, 4):
            q = Qd[:b].contiguous()
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            routes = {"fp32_filtered": lambda: corpus.search_device(q, k, eta, 0.0, ids, sc, filter=f),
                      "int8_filtered": lambda: corpus.search_approx_filtered_device(q, k, eta, 0.0, f, None, True, ids, sc)}
            if frac >= 1.0:
                routes["int8_unfiltered"] = lambda: corpus.search_approx_device(q, k, eta, 0.0, None, True, ids, sc)
            res = _alternate(torch, routes, a.rounds, a.iters, a.warmup)
            rec = {"case": "list", "fraction": frac, "n_allowed": n_a, "k": k, "batch": b, "n": n, "dim": d, "iters": a.iters,
                   "rounds": a.rounds, "recall_mean_min": recall}
            print(f"  batch {b}")
            for key, (med, lo, hi) in res.items():
                print(f"    {key:<16} {med:9.4f} ms   ({lo:.4f} - {hi:.4f})   [device, whole search]")
                rec[key + "_ms"], rec[key + "_spread_ms"] = round(med, 5), [round(lo, 5), round(hi, 5)]
            for key, nbytes in (("fp32_filtered", n_a * d * 4 + 4 * n_a + b * d * 4), ("int8_filtered", n_a * (d + 4) + 4 * n_a + b * d * 4)):
                ms, launches = _scan_ms(torch, eng, routes[key], a.iters)
                rate = nbytes / (ms * 1e-3) if ms > 0 else 0.0
                rec[key + "_scan_ms"], rec[key + "_scan_share_of_hbm_peak"] = round(ms, 5), round(rate / HBM_PEAK, 4)
                print(f"    {key:<16} scan bracket {ms:9.4f} ms over {launches} calls, one pass: {rate / 1e12:.3f} TB/s algorithmic = "
                      f"{rate / HBM_PEAK:.3f} of the 8 TB/s peak")
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()


def part_ivf(a, np, torch, eng, X, Q, out):
    from dewi.ivf import IVFIndex, PROBE_GROUP
    n, d, k, eta = a.n, a.dim, a.k, a.eta
    rs = np.random.RandomState(0)
    cols = {"dewi": rs.rand(n), "ht_mean": rs.rand(n), "hi_mean": rs.rand(n)}
    idx = IVFIndex(d, "cosine", nlist=a.nlist, train_iters=a.train_iters, int8_codes=True)
    idx.add_batch_columns([f"doc_{i:08d}" for i in range(n)], X, cols)
    t = time.perf_counter()
    idx.build()
    torch.cuda.synchronize()
    sizes = idx.cell_sizes
    print(f"build {time.perf_counter() - t:.2f} s; {a.nlist} cells of {int(sizes.min())}-{int(sizes.max())} rows "
          f"(median {int(np.median(sizes))})")
    corpus, st = idx._corpus, idx._ivf
    Qd = torch.from_numpy(Q).cuda()
    exact_ids = corpus.search_device(Qd, k, 0.0, 0.0)[0].cpu().numpy()
    c = 2 * k
    for npb in [int(x) for x in a.nprobe.split(",")]:
        rec_fp32 = _recall(np, idx.search_device(Qd, k, 0.0, 0.0, nprobe=npb, approx=False)[0].cpu().numpy(), exact_ids, k)
        rec_i8 = _recall(np, idx.search_device(Qd, k, 0.0, 0.0, nprobe=npb, approx=True)[0].cpu().numpy(), exact_ids, k)
        print(f"\nnprobe {npb}: recall@{k} vs the exact search (mean, min): fp32 probe {rec_fp32}, int8 probe {rec_i8}")
        for b in (1, 32):
            q = Qd[:b].contiguous()
            routes = {"fp32_probe": lambda: idx.search_device(q, k, eta, 0.0, nprobe=npb, approx=False),
                      "int8_probe": lambda: idx.search_device(q, k, eta, 0.0, nprobe=npb, approx=True)}
            res = _alternate(torch, routes, a.rounds, a.iters, a.warmup)
            coarse = lambda: st.coarse.search_device(q, npb, 0.0, 0.0, candidates=npb)      # noqa: E731
            coarse_ms = _events(torch, coarse, a.iters)
            pids = coarse()[0]
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.iters):
                n_union, n_allowed, stride = idx._prepare_probe(pids, b, npb)
            prep_ms = (time.perf_counter() - t) * 1e3 / a.iters
            if min(n_allowed) < c:
                print(f"  batch {b}: a probe holds fewer than {c} rows: no split")
                continue
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            scans = {"fp32_probe": lambda: idx._search_groups(q, n_union, n_allowed, stride, k, c, None, 0, eta, 0.0, ids, sc),
                     "int8_probe": lambda: idx._search_groups_i8(q, n_union, n_allowed, stride, k, c, True, eta, 0.0, ids, sc)}
            scan_res = _alternate(torch, scans, a.rounds, a.iters, 2)
            reach = float(np.mean(n_allowed)) if b == 1 else float(np.mean(n_union))
            rec = {"case": "ivf", "nprobe": npb, "batch": b, "group": PROBE_GROUP, "rows_reached": round(reach, 1), "k": k,
                   "recall_fp32_mean_min": rec_fp32, "recall_int8_mean_min": rec_i8, "coarse_ms": round(coarse_ms, 5),
                   "prepare_ms": round(prep_ms, 5), "iters": a.iters, "rounds": a.rounds}
            print(f"  batch {b}: {reach:.0f} rows reached; coarse {coarse_ms:.4f} ms, prepare {prep_ms:.4f} ms [host clock]")
            for key in routes:
                med, lo, hi = res[key]
                smed, slo, shi = scan_res[key]
                rec[key + "_ms"], rec[key + "_spread_ms"] = round(med, 5), [round(lo, 5), round(hi, 5)]
                rec[key + "_scan_select_ms"], rec[key + "_scan_select_spread_ms"] = round(smed, 5), [round(slo, 5), round(shi, 5)]
                print(f"    {key:<12} {med:9.4f} ms per search ({lo:.4f} - {hi:.4f});  scan + select {smed:9.4f} ms ({slo:.4f} - {shi:.4f})")
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("lists", "ivf"), required=True)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--fractions", default="0.01,0.1,0.5,1.0")
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", default="1,4,16,64")
    ap.add_argument("--train-iters", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import numpy as np
    import torch
    from corpora import embedding_like
    from dewi import _engine as eng

    X, Q, _, _ = embedding_like(a.n, a.dim, 3)
    out = open(a.json, "w") if a.json else None
    print(f"corpus {a.n} x {a.dim} fp32 embedding_like, k {a.k}, eta {a.eta}, {a.rounds} rounds of {a.iters} calls")
    (part_lists if a.part == "lists" else part_ivf)(a, np, torch, eng, X, Q, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()

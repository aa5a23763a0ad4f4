"""IVFIndex at 1 M x 768 fp32 on a clustered corpus: time per search against nprobe, split by stage, with the recall.

The corpus is 1 024 gaussian centres + unit noise, rows normalised (an isotropic corpus has no cells to find); queries are
corpus rows + 0.05 noise.  For nprobe in --nprobe and for one query and batches of 32 it prints: the rows the probe reaches
(|F_j| for one query, |U| per group of 8 for a batch), recall@k against the exact search OF THE SAME RUN AND CORPUS (same k,
eta), the time per search call (events around `iters` back-to-back calls; every call synchronises once inside
dewi_ivf_probe_prepare), and the split: coarse (events, enqueue only), prepare (wall clock, the read-back included),
list scan + select (events, on a prepared buffer).  The exact search is timed the same way first; build time is wall clock.

    python scripts/bench_ivf.py [--n 1048576] [--dim 768] [--nlist 1024] [--nprobe 1,4,16,64] [--k 10] [--iters 50] [--json out.jsonl]
"""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))


def _events(torch, fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--centres", type=int, default=1024)
    ap.add_argument("--nprobe", default="1,4,16,64")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train-iters", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dewi.ivf import IVFIndex, PROBE_GROUP

    n, d, k, eta = a.n, a.dim, a.k, a.eta
    gen = torch.Generator(device="cuda").manual_seed(0)
    cen = torch.randn(a.centres, d, generator=gen, device="cuda")
    emb = torch.empty(n, d, dtype=torch.float32, device="cuda")
    for s in range(0, n, 1 << 16):
        m = min(1 << 16, n - s)
        lab = torch.randint(0, a.centres, (m,), generator=gen, device="cuda")
        blk = cen[lab] + torch.randn(m, d, generator=gen, device="cuda")
        emb[s:s + m] = blk / torch.linalg.vector_norm(blk, dim=1, keepdim=True)
    rows = torch.randperm(n, generator=gen, device="cuda")[:64]
    Q = emb[rows] + 0.05 * torch.randn(64, d, generator=gen, device="cuda")
    Q = (Q / torch.linalg.vector_norm(Q, dim=1, keepdim=True)).contiguous()
    cols = {"dewi": torch.rand(n, generator=gen, device="cuda", dtype=torch.float64),
            "ht_mean": torch.rand(n, generator=gen, device="cuda", dtype=torch.float64),
            "hi_mean": torch.rand(n, generator=gen, device="cuda", dtype=torch.float64)}

    idx = IVFIndex(d, "cosine", nlist=a.nlist, train_iters=a.train_iters)
    idx.add_batch_columns([f"doc_{i:08d}" for i in range(n)], emb, cols)
    t = time.perf_counter()
    super(IVFIndex, idx).build()
    torch.cuda.synchronize()
    t_exact = time.perf_counter() - t
    t = time.perf_counter()
    idx._build_ivf()
    torch.cuda.synchronize()
    t_ivf = time.perf_counter() - t
    sizes = idx.cell_sizes
    print(f"build: corpus {t_exact:.3f} s, k-means ({a.train_iters} rounds) + assignment + cell lists {t_ivf:.3f} s; "
          f"{a.nlist} cells of {int(sizes.min())}-{int(sizes.max())} rows (median {int(np.median(sizes))})")
    out = open(a.json, "w") if a.json else None
    if out:
        out.write(json.dumps({"case": "build", "corpus_s": round(t_exact, 3), "ivf_s": round(t_ivf, 3), "nlist": a.nlist,
                              "cell_min": int(sizes.min()), "cell_max": int(sizes.max())}) + "\n")

    corpus, st = idx._corpus, idx._ivf
    exact_ids, _ = corpus.search_device(Q, k, eta, 0.0)
    exact_ids = exact_ids.cpu().numpy()
    exact_ms = {}
    for b in (1, 32):
        q = Q[:b].contiguous()
        ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
        sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
        for _ in range(a.warmup):
            corpus.search_device(q, k, eta, 0.0, ids, sc)
        torch.cuda.synchronize()
        exact_ms[b] = _events(torch, lambda: corpus.search_device(q, k, eta, 0.0, ids, sc), a.iters)
        print(f"exact search, {b:>2} queries: {exact_ms[b]:.4f} ms per call ({corpus.scan_kernel_name(b, k)})")
        if out:
            out.write(json.dumps({"case": "exact", "batch": b, "ms_per_search": round(exact_ms[b], 5)}) + "\n")

    print(f"{'nprobe':>6} {'B':>3} {'rows':>8} {'recall':>7} {'ms/search':>10} {'coarse':>8} {'prepare':>8} {'scan+sel':>9} {'vs exact':>9}")
    for npb in [int(x) for x in a.nprobe.split(",")]:
        got = idx.search_device(Q, k, eta, 0.0, nprobe=npb)[0].cpu().numpy()
        recall = float(np.mean([len(set(got[j].tolist()) & set(exact_ids[j].tolist())) / k for j in range(64)]))
        for b in (1, 32):
            q = Q[:b].contiguous()
            c = 2 * k
            run = lambda: idx.search_device(q, k, eta, 0.0, nprobe=npb)      # noqa: E731
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            ms = _events(torch, run, a.iters)
            coarse = lambda: st.coarse.search_device(q, npb, 0.0, 0.0, candidates=npb)      # noqa: E731
            coarse_ms = _events(torch, coarse, a.iters)
            pids = coarse()[0]
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.iters):
                n_union, n_allowed, stride = idx._prepare_probe(pids, b, npb)
            prep_ms = (time.perf_counter() - t) * 1e3 / a.iters
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            scan = lambda: idx._search_groups(q, n_union, n_allowed, stride, k, c, None, 0, eta, 0.0, ids, sc)      # noqa: E731
            scan()
            torch.cuda.synchronize()
            scan_ms = _events(torch, scan, a.iters)
            reach = float(np.mean(n_allowed)) if b == 1 else float(np.mean(n_union))
            rel = ms / exact_ms[b]
            print(f"{npb:>6} {b:>3} {reach:>8.0f} {recall:>7.3f} {ms:>10.4f} {coarse_ms:>8.4f} {prep_ms:>8.4f} {scan_ms:>9.4f}   x{rel:.3f}")
            if out:
                out.write(json.dumps({"case": "ivf", "nprobe": npb, "batch": b, "group": PROBE_GROUP, "rows_reached": round(reach, 1),
                                      "recall_at_k": round(recall, 4), "ms_per_search": round(ms, 5), "coarse_ms": round(coarse_ms, 5),
                                      "prepare_ms": round(prep_ms, 5), "scan_select_ms": round(scan_ms, 5),
                                      "vs_exact": round(rel, 4)}) + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()

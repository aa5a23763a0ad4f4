"""Diverse (MMR) search at 1 M x 768 fp32: device time of `search_diverse_device` against `search_device(..., candidates=c)` of
the same build, alternating in one process, and the re-rank kernel on its own.

The corpus is isotropic (normalised gaussian rows) with every 16th row given a near-copy, the queries are perturbed rows, so
the pools hold near-duplicates as a real text-image corpus does.  Cases: k = 10 with c = 40 and k = 100 with c = 400, batches
of 1 / 32 / 256.

Per case, `rounds` rounds of `iters` calls each, the three measurements alternating round by round:
  search          search_device(q, k, candidates=c): scan + select / blend / top-k, events around back-to-back enqueues [device]
  diverse         search_diverse_device(q, k, candidates=c): the prefill, candidates_device (scan + select -> records) and
                  dewi_diverse_rerank, the same way                                                                    [device]
  re-rank         dewi_diverse_rerank alone on the records of the batch, the same way                                  [device]
Medians over the rounds, with the min-max spread of the rounds.

    python scripts/bench_diverse.py [--n 1048576] [--dim 768] [--cases 10:40,100:400] [--batches 1,32,256] [--iters 20]
                                    [--rounds 5] [--mmr-lambda 0.5] [--json out.jsonl]
"""
import argparse
import json
import statistics
import sys
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


def _med(xs):
    return statistics.median(xs), min(xs), max(xs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--cases", default="10:40,100:400", help="k:c pairs")
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--mmr-lambda", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng
    from dewi import _native as nat

    n, d, eta, lam = a.n, a.dim, a.eta, a.mmr_lambda
    gen = torch.Generator(device="cuda").manual_seed(0)
    emb = torch.empty(n, d, dtype=torch.float32, device="cuda")
    for s in range(0, n, 1 << 16):
        m = min(1 << 16, n - s)
        blk = torch.randn(m, d, generator=gen, device="cuda")
        blk[1::16] = blk[0::16][: blk[1::16].shape[0]] + 0.02 * torch.randn(blk[1::16].shape, generator=gen, device="cuda")
        emb[s:s + m] = blk / torch.linalg.vector_norm(blk, dim=1, keepdim=True)
    dewi32 = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
    ent32 = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
    corpus = eng.DeviceCorpus(emb, dewi32, ent32, "cosine")
    lib = corpus._lib
    out = open(a.json, "w") if a.json else None
    print(f"corpus {n} x {d} fp32 (every 16th row has a near-copy), eta {eta}, mmr_lambda {lam}")

    for case in a.cases.split(","):
        k, c = (int(x) for x in case.split(":"))
        for b in (int(x) for x in a.batches.split(",")):
            src = torch.randint(0, n, (b,), generator=gen, device="cuda")
            q = (emb[src] + 0.3 / d ** 0.5 * torch.randn(b, d, generator=gen, device="cuda")).contiguous()
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            recs = corpus.candidates_device(q, c).clone()
            search = lambda: corpus.search_device(q, k, eta, 0.0, ids, sc, candidates=c)                               # noqa: E731
            diverse = lambda: corpus.search_diverse_device(q, k, eta, 0.0, lam, c, None, ids, sc)                     # noqa: E731
            rerank = lambda: nat.check(lib.dewi_diverse_rerank(nat.ptr(emb), 0, n, d, nat.ptr(recs), b, c, k, eta, 0.0, lam,  # noqa: E731
                                                               float("inf"), 0, nat.ptr(ids), nat.ptr(sc), None, None, 0,
                                                               nat.stream_ptr()))
            for _ in range(a.warmup):
                search(), diverse(), rerank()
            torch.cuda.synchronize()
            r = {"search": [], "diverse": [], "rerank": []}
            for _ in range(a.rounds):
                r["search"].append(_events(torch, search, a.iters))
                r["diverse"].append(_events(torch, diverse, a.iters))
                r["rerank"].append(_events(torch, rerank, a.iters))
            rec = {"case": "diverse", "k": k, "c": c, "batch": b, "n": n, "dim": d, "mmr_lambda": lam, "iters": a.iters,
                   "rounds": a.rounds, "scan_kernel": corpus.scan_kernel_name(b, k, candidates=c)}
            print(f"\nk {k}, c {c}, batch {b} (scan kernel: {rec['scan_kernel']})")
            for key, label in (("search", "search(candidates=c), device"), ("diverse", "search_diverse, device"),
                               ("rerank", "  dewi_diverse_rerank alone")):
                med, lo, hi = _med(r[key])
                print(f"  {label:<32} {med:9.4f} ms   ({lo:.4f} - {hi:.4f})")
                rec[key + "_ms"] = round(med, 5)
                rec[key + "_spread_ms"] = [round(lo, 5), round(hi, 5)]
            rec["vs_search"] = round(rec["diverse_ms"] / rec["search_ms"], 4)
            print(f"  diverse / search = x{rec['vs_search']:.3f}")
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()

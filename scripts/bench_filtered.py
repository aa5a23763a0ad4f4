"""Filtered exact search at 1 M x 768 fp32: time per search against the fraction of the corpus the filter allows.

For each filter — none (the unfiltered search, same run), all rows, random masks of selectivity 0.5 / 0.1 / 0.01 / 0.001,
one contiguous block of 10 % — and for batches of 1 and 32 queries it prints the wall time per search call (events around
`iters` back-to-back enqueues on one stream), the scan kernel's own time (dewi_timing_read), the bytes the scan reads (the
allowed rows plus the 4-byte list entries) and what fraction of the 8 TB/s HBM peak that is over the scan time.

    python scripts/bench_filtered.py [--n 1048576] [--dim 768] [--k 10] [--iters 50] [--warmup 10] [--json out.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))

PEAK_BPS = 8e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng
    from dewi import _native as nat

    lib = nat.load_library()
    torch.manual_seed(0)
    n, d, k = a.n, a.dim, a.k
    emb = torch.randn(n, d, dtype=torch.float32, device="cuda")
    nat.check(lib.dewi_normalize_rows_f32(nat.ptr(emb), nat.ptr(emb), n, d, nat.stream_ptr()))
    dewi32 = torch.rand(n, dtype=torch.float32, device="cuda")
    ent32 = torch.rand(n, dtype=torch.float32, device="cuda")
    corpus = eng.DeviceCorpus(emb, dewi32, ent32, "cosine")
    Q = torch.randn(32, d, dtype=torch.float32, device="cuda")

    gen = torch.Generator(device="cuda").manual_seed(1)
    cases = [("none", None), ("all", torch.ones(n, dtype=torch.bool, device="cuda"))]
    for sel in (0.5, 0.1, 0.01, 0.001):
        cases.append((f"random_{sel:g}", torch.rand(n, generator=gen, device="cuda") < sel))
    block = torch.zeros(n, dtype=torch.bool, device="cuda")
    block[n // 3: n // 3 + n // 10] = True
    cases.append(("block_0.1", block))

    out = open(a.json, "w") if a.json else None
    print(f"{'filter':>14} {'rows':>9} {'B':>3} {'ms/search':>10} {'scan ms':>8} {'MB read':>8} {'of 8 TB/s':>9}")
    base = {}
    for name, mask in cases:
        f = corpus.make_filter(mask) if mask is not None else None
        n_a = n if f is None else f.n_allowed
        for b in (1, 32):
            q = Q[:b].contiguous()
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            for _ in range(a.warmup):
                corpus.search_device(q, k, 0.3, 0.0, ids, sc, filter=f)
            torch.cuda.synchronize()
            eng.timing(1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                corpus.search_device(q, k, 0.3, 0.0, ids, sc, filter=f)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.iters
            scan_ms, _ = eng.timing_read()
            eng.timing(0)
            nbytes = n_a * d * 4 + (0 if f is None else n_a * 4)
            frac = nbytes / (scan_ms * 1e-3) / PEAK_BPS if scan_ms > 0 else 0.0
            if name == "none":
                base[b] = (ms, scan_ms)
            rel = ms / base[b][0] if b in base else float("nan")
            print(f"{name:>14} {n_a:>9} {b:>3} {ms:>10.4f} {scan_ms:>8.4f} {nbytes / 1e6:>8.1f} {frac:>9.3f}   x{rel:.3f} of unfiltered")
            if out:
                out.write(json.dumps({"filter": name, "n_allowed": n_a, "batch": b, "ms_per_search": round(ms, 5),
                                      "scan_ms": round(scan_ms, 5), "bytes_read": nbytes, "frac_of_peak": round(frac, 4),
                                      "vs_unfiltered": round(rel, 4), "kernel": corpus.scan_kernel_name(b, k)}) + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()

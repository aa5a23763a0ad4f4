"""Range search at 1 M x 768 fp32, one query: device time split into scan, count and collect, the whole call through Python,
and the one-query top-10 search of the same build as the reference point, alternating in the same run.

The corpus is isotropic (normalised gaussian rows): the query's similarities are ~N(0, 1/d), so thresholds that return about
10, 1 000 and 100 000 rows exist and are read off the query's own score distribution (the exact counts are printed).

Per threshold, `rounds` rounds of `iters` calls each, the top-10 search and the range search alternating round by round:
  search        dewi_knn_rerank_f32 (k = 10), events around back-to-back enqueues                       [device]
  its scan      the library's own brackets around the corpus pass (dewi_timing_enable)                  [device]
  count call    dewi_knn_range_count — dense scan + range_count + range_offsets — events, enqueue only  [device]
  its scan      the library's brackets around the dense corpus pass                                     [device]
  count         count call minus its scan: range_count + range_offsets                                  [device]
  collect       dewi_knn_range_collect on the workspace the count left, events, enqueue only            [device]
  whole call    DeviceCorpus.range_search_device (sorted and unsorted): wall clock around calls that each synchronise once
                for the counts and once at the end                                                      [host]
Medians over the rounds, with the min-max spread of the rounds.

    python scripts/bench_range.py [--n 1048576] [--dim 768] [--targets 10,1000,100000] [--iters 50] [--rounds 5] [--json out.jsonl]
"""
import argparse
import json
import statistics
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


def _wall(torch, fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / iters


def _med(xs):
    return statistics.median(xs), min(xs), max(xs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--targets", default="10,1000,100000")
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng
    from dewi import _native as nat

    n, d, eta, k = a.n, a.dim, a.eta, 10
    gen = torch.Generator(device="cuda").manual_seed(0)
    emb = torch.empty(n, d, dtype=torch.float32, device="cuda")
    for s in range(0, n, 1 << 16):
        m = min(1 << 16, n - s)
        blk = torch.randn(m, d, generator=gen, device="cuda")
        emb[s:s + m] = blk / torch.linalg.vector_norm(blk, dim=1, keepdim=True)
    q = torch.randn(1, d, generator=gen, device="cuda")
    q = (q / torch.linalg.vector_norm(q, dim=1, keepdim=True)).contiguous()
    dewi32 = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
    ent32 = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
    corpus = eng.DeviceCorpus(emb, dewi32, ent32, "cosine")
    lib = corpus._lib
    sp = nat.SPACE_CODES["cosine"]

    # thresholds from the query's own score distribution (the library's scores: a range search below every score, unsorted)
    _, _, sims, _ = corpus.range_search_device(q, -2.0, eta, 0.0, sort=False)
    ordered = torch.sort(sims, descending=True).values
    targets = [int(x) for x in a.targets.split(",")]
    taus = [float(ordered[min(t, n) - 1]) for t in targets]
    del sims, ordered

    ids = torch.empty((1, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((1, k), dtype=torch.float32, device="cuda")
    search = lambda: corpus.search_device(q, k, eta, 0.0, ids, sc)      # noqa: E731
    print(f"corpus {n} x {d} fp32, one query, eta {eta}; top-{k} search kernel: {corpus.scan_kernel_name(1, k)}; "
          f"dense form of the same kernel for the range scan: {corpus.scan_kernel_name(1, k, candidates=257)}")
    out = open(a.json, "w") if a.json else None

    ws_bytes = int(lib.dewi_knn_range_workspace_bytes(n, d, 0, 1))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    counts = torch.empty(1, dtype=torch.int64, device="cuda")

    def timed_scan(fn, iters):
        """(events ms per call, the library's own bracket around the corpus pass) of `iters` calls of fn: two passes, because
        the brackets' event records cost stream time themselves."""
        ms = _events(torch, fn, iters)
        eng.timing(1)
        _events(torch, fn, iters)
        scan_ms, launches = eng.timing_read()
        eng.timing(0)
        assert launches == iters, (launches, iters)
        return ms, scan_ms

    for target, tau in zip(targets, taus):
        thr = torch.full((1,), tau, dtype=torch.float32, device="cuda")
        count = lambda: nat.check(lib.dewi_knn_range_count(nat.ptr(emb), 0, n, d, None, 0, nat.ptr(q), 1, nat.ptr(thr), sp,      # noqa: E731
                                                           nat.ptr(counts), nat.ptr(ws), ws_bytes, nat.stream_ptr()))
        count()
        m = int(counts.item())
        lims = torch.tensor([0, m], dtype=torch.int64, device="cuda")
        rows = torch.empty(max(m, 1), dtype=torch.int64, device="cuda")
        o_sims = torch.empty(max(m, 1), dtype=torch.float32, device="cuda")
        o_sc = torch.empty(max(m, 1), dtype=torch.float32, device="cuda")
        collect = lambda: nat.check(lib.dewi_knn_range_collect(nat.ptr(ws), ws_bytes, n, 1, nat.ptr(thr), nat.ptr(lims), m,      # noqa: E731
                                                               nat.ptr(dewi32), nat.ptr(ent32), eta, 0.0, nat.ptr(rows),
                                                               nat.ptr(o_sims), nat.ptr(o_sc), nat.stream_ptr()))
        whole = lambda: corpus.range_search_device(q, thr, eta, 0.0)                     # noqa: E731
        whole_unsorted = lambda: corpus.range_search_device(q, thr, eta, 0.0, sort=False)  # noqa: E731
        for _ in range(a.warmup):
            search(), count(), collect(), whole(), whole_unsorted()
        torch.cuda.synchronize()
        r = {key: [] for key in ("search", "search_scan", "count_call", "dense_scan", "count", "collect", "whole", "whole_unsorted",
                                 "search_wall")}
        for _ in range(a.rounds):
            ms, scan_ms = timed_scan(search, a.iters)
            r["search"].append(ms)
            r["search_scan"].append(scan_ms)
            ms, scan_ms = timed_scan(count, a.iters)
            r["count_call"].append(ms)
            r["dense_scan"].append(scan_ms)
            r["count"].append(ms - scan_ms)
            r["collect"].append(_events(torch, collect, a.iters))
            r["search_wall"].append(_wall(torch, lambda: (search(), torch.cuda.current_stream().synchronize()), a.iters))
            r["whole"].append(_wall(torch, whole, a.iters))
            r["whole_unsorted"].append(_wall(torch, whole_unsorted, a.iters))
        print(f"\nthreshold {tau:.6f}: {m} rows (target {target})")
        rec = {"case": "range", "rows": m, "threshold": tau, "n": n, "dim": d, "iters": a.iters, "rounds": a.rounds}
        for key, label in (("search", "top-10 search, device"), ("search_scan", "  its corpus pass (list form)"),
                           ("count_call", "range count call, device"), ("dense_scan", "  its corpus pass (dense form)"),
                           ("count", "  range_count + range_offsets"), ("collect", "range collect, device"),
                           ("search_wall", "top-10 search, host (one sync)"), ("whole", "range search, host, sorted"),
                           ("whole_unsorted", "range search, host, unsorted")):
            med, lo, hi = _med(r[key])
            print(f"  {label:<34} {med:9.4f} ms   ({lo:.4f} - {hi:.4f})")
            rec[key + "_ms"] = round(med, 5)
            rec[key + "_spread_ms"] = [round(lo, 5), round(hi, 5)]
        dev = statistics.median(r["count_call"]) + statistics.median(r["collect"])
        rec["range_device_ms"] = round(dev, 5)
        rec["vs_search_device"] = round(dev / statistics.median(r["search"]), 4)
        print(f"  range device total (count call + collect) {dev:.4f} ms = x{rec['vs_search_device']:.3f} of the top-10 search")
        if out:
            out.write(json.dumps(rec) + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()

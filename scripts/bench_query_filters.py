"""Per-query filters at 1 M x 768 fp32, B = 32: one batch where every query has its own allow-list.

For each case — overlapping lists (50 % of the rows shared by all + 5 % of each query's own), disjoint 10 % lists,
identical 50 % lists, and one list per query that covers every row — it prints the wall time per call (events around
`iters` back-to-back enqueues on one stream) and the scan kernels' own time (dewi_timing_read) of:
  qf      the per-query-filter batch (one QMASK pass over the union U per 8 queries),
  union   the single-list batch over the same U (one filter for all: the answers are NOT per query, the speed yardstick),
  singles 32 single-list calls, one per query, on its own list.

    python scripts/bench_query_filters.py [--n 1048576] [--dim 768] [--k 10] [--iters 20] [--warmup 5] [--json out.jsonl]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng
    from dewi import _native as nat

    lib = nat.load_library()
    torch.manual_seed(0)
    n, d, k, b = a.n, a.dim, a.k, a.b
    emb = torch.randn(n, d, dtype=torch.float32, device="cuda")
    nat.check(lib.dewi_normalize_rows_f32(nat.ptr(emb), nat.ptr(emb), n, d, nat.stream_ptr()))
    dewi32 = torch.rand(n, dtype=torch.float32, device="cuda")
    ent32 = torch.rand(n, dtype=torch.float32, device="cuda")
    corpus = eng.DeviceCorpus(emb, dewi32, ent32, "cosine")
    Q = torch.randn(b, d, dtype=torch.float32, device="cuda")

    gen = torch.Generator(device="cuda").manual_seed(1)
    shared = torch.rand(n, generator=gen, device="cuda") < 0.5
    overlap = shared[None, :] | (torch.rand(b, n, generator=gen, device="cuda") < 0.05)
    part = torch.randint(0, 10, (n,), generator=gen, device="cuda")
    disjoint = torch.stack([part == (j % 10) for j in range(b)])
    cases = [("overlap_50+5", overlap), ("disjoint_0.1", disjoint),
             ("identical_0.5", shared[None, :].expand(b, n).contiguous()),
             ("all_rows", torch.ones(b, n, dtype=torch.bool, device="cuda"))]

    ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
    sc = torch.empty((b, k), dtype=torch.float32, device="cuda")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        eng.timing(1)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        scan_ms, _ = eng.timing_read()
        eng.timing(0)
        return t0.elapsed_time(t1) / a.iters, scan_ms

    out = open(a.json, "w") if a.json else None
    print(f"{'case':>14} {'|U|':>8} {'mean|F|':>8} {'qf ms':>8} {'scan':>8} {'union ms':>9} {'scan':>8} "
          f"{'32 singles':>11} {'scan':>8} {'qf/union':>9} {'qf/singles':>10}")
    for name, masks in cases:
        qf = corpus.make_query_filters(masks)
        fu = corpus.make_filter(masks.any(dim=0))
        singles = [corpus.make_filter(masks[j]) for j in range(b)]
        qf_ms, qf_scan = timed(lambda: corpus.search_device(Q, k, 0.3, 0.0, ids, sc, filter=qf))
        un_ms, un_scan = timed(lambda: corpus.search_device(Q, k, 0.3, 0.0, ids, sc, filter=fu))

        def all_singles():
            for j in range(b):
                corpus.search_device(Q[j:j + 1], k, 0.3, 0.0, ids[j:j + 1], sc[j:j + 1], filter=singles[j])
        si_ms, si_scan = timed(all_singles)
        mean_f = float(qf.n_allowed.mean())
        print(f"{name:>14} {qf.n_union:>8} {mean_f:>8.0f} {qf_ms:>8.4f} {qf_scan:>8.4f} {un_ms:>9.4f} {un_scan:>8.4f} "
              f"{si_ms:>11.4f} {si_scan:>8.4f} {qf_ms / un_ms:>9.3f} {qf_ms / si_ms:>10.3f}")
        if out:
            out.write(json.dumps({"case": name, "n_union": qf.n_union, "mean_n_allowed": round(mean_f, 1), "batch": b, "k": k,
                                  "qf_ms": round(qf_ms, 5), "qf_scan_ms": round(qf_scan, 5), "union_ms": round(un_ms, 5),
                                  "union_scan_ms": round(un_scan, 5), "singles_ms": round(si_ms, 5),
                                  "singles_scan_ms": round(si_scan, 5), "qf_vs_union": round(qf_ms / un_ms, 4),
                                  "qf_vs_singles": round(qf_ms / si_ms, 4)}) + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()

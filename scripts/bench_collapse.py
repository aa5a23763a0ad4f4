"""Collapsed search at 1 M x 768 fp32 against the stages it replaces, in one process, the routes alternating round by round
(medians of ``rounds`` rounds of ``iters`` back-to-back calls between device events, with the min-max spread of the rounds).

The corpus is made on the device: gaussian unit rows, one cluster of ``--cluster`` exact copies; the labels are random groups
of mean size ``--group-size`` plus the cluster as one group.  Queries are rows of the corpus plus noise, query 0 inside the
cluster.

  --part kernel    ``dewi_collapse_rerank`` against ``dewi_merge_rerank`` on the SAME candidate records (per_group 1 and c: the
                   second folds nothing and returns the merge's answer), c in --cuts, 1 and 256 queries
  --part search    ``search_collapsed_device(candidates=c)`` against ``search_device(candidates=c)``, 1 and 256 queries
  --part filtered  the same two under a random allow-list of --fraction of the rows, 1 and 32 queries

    python scripts/bench_collapse.py --part kernel|search|filtered [--n 1048576] [--dim 768] [--k 10] [--json out.jsonl]

Phases of the kernel: build csrc/collapse.hip with -DDEWI_COLLAPSE_STOP_AFTER=1|2|3 (it then returns after the records, the
sort, the rank inside the group), link it with the library's other objects into a library of its own and run ``--part kernel``
with ``DEWI_HIP_LIB`` pointing at it; the differences between the builds are the phases (profiles/r16/collapse/).
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


def _report(rec, res, base, out):
    for key, (med, lo, hi) in res.items():
        rec[key + "_ms"], rec[key + "_spread_ms"] = round(med, 5), [round(lo, 5), round(hi, 5)]
        ratio = "" if key == base else f"   x{med / res[base][0]:.2f} of {base}"
        print(f"    {key:<22} {med:9.4f} ms   ({lo:.4f} - {hi:.4f}){ratio}")
        if key != base:
            rec[key + "_over_" + base] = round(med / res[base][0], 3)
    if out:
        out.write(json.dumps(rec) + "\n")
        out.flush()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "search", "filtered"), required=True)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--cuts", default="40,400,1024,2048")
    ap.add_argument("--cluster", type=int, default=1500)
    ap.add_argument("--group-size", type=int, default=8)
    ap.add_argument("--fraction", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng

    n, d, k, eta = a.n, a.dim, a.k, a.eta
    gen = torch.Generator(device="cuda").manual_seed(11)
    emb = torch.randn((n, d), device="cuda", generator=gen)
    emb /= emb.norm(dim=1, keepdim=True)
    emb[: a.cluster] = emb[0]
    labels = torch.randint(0, max(1, n // a.group_size), (n,), device="cuda", generator=gen, dtype=torch.int64)
    labels[: a.cluster] = n                                       # the cluster: a group of its own
    corpus = eng.DeviceCorpus(emb, torch.rand(n, device="cuda", generator=gen), torch.rand(n, device="cuda", generator=gen))
    groups = corpus.make_groups(labels)
    rows = torch.randint(a.cluster, n, (256,), device="cuda", generator=gen)
    rows[0] = 0
    Q = (emb[rows] + 0.3 / d ** 0.5 * torch.randn((256, d), device="cuda", generator=gen)).contiguous()
    out = open(a.json, "w") if a.json else None
    cuts = [int(x) for x in a.cuts.split(",")]
    print(f"corpus {n} x {d} fp32 gaussian, one cluster of {a.cluster} copies, {groups.n_groups} groups; k {k}, eta {eta}, "
          f"{a.rounds} rounds of {a.iters} calls; part {a.part}")
    f = corpus.make_filter(torch.rand(n, device="cuda", generator=gen) < a.fraction) if a.part == "filtered" else None
    for c in cuts:
        for b in ((1, 32) if a.part == "filtered" else (1, 256)):
            q = Q[:b].contiguous()
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            hits = torch.empty((b, k), dtype=torch.int32, device="cuda")
            cnt = torch.empty(b, dtype=torch.int32, device="cuda")
            rec = {"part": a.part, "c": c, "batch": b, "k": k, "n": n, "dim": d, "iters": a.iters, "rounds": a.rounds}
            iters = a.iters if b == 1 or a.part == "kernel" else max(5, a.iters // 5)
            if a.part == "kernel":
                recs = corpus.candidates_device(q, c).clone()
                lists = recs.unsqueeze(0)
                routes = {"merge_rerank": lambda: eng.merge_rerank_device(lists, c, k, eta, 0.0, ids, sc),
                          "collapse_per_group_1": lambda: corpus.collapse_rerank_device(recs, k, eta, 0.0, groups, 1, ids, sc, hits, cnt),
                          "collapse_nothing_folded": lambda: corpus.collapse_rerank_device(recs, k, eta, 0.0, groups, c, ids, sc, hits, cnt)}
                base = "merge_rerank"
                corpus.collapse_rerank_device(recs, k, eta, 0.0, groups, 1, ids, sc, hits, cnt)
                torch.cuda.synchronize()
                rec["results_of_query_0"] = int(cnt[0].item())
            else:
                routes = {"search": lambda: corpus.search_device(q, k, eta, 0.0, ids, sc, candidates=c, filter=f),
                          "search_collapsed": lambda: corpus.search_collapsed_device(q, k, eta, 0.0, groups, 1, c, f, False, True, ids, sc, hits)}
                base = "search"
                if f is not None:
                    rec["n_allowed"] = f.n_allowed
            print(f"  c {c}, batch {b}" + (f", list of {f.n_allowed} rows" if f is not None else ""))
            _report(rec, _alternate(torch, routes, a.rounds, iters, a.warmup), base, out)
    if out:
        out.close()


if __name__ == "__main__":
    main()

"""The approximate binary route at 1 M x 768 against the int8 route and the exact fp32 search of the same build, in one
process, the routes alternating round by round.

The corpus is ``tests/corpora.embedding_like`` (clustered unit rows, 32 queries near rows of the corpus: the one the int8
figures use).  Per k (10, 100) and batch (1, 4):
  exact            search_device on the fp32 rows                                        events around back-to-back enqueues [device]
  int8             search_approx_device (cut 2k, re-scored): ``search(approx=True)``      the same way                        [device]
  binary c         search_binary_device at the cuts 128 / 256 / 512 / 1024 (re-scored)    the same way                        [device]
  scan kernels     the library's own brackets around the corpus scan (dewi_timing_enable): exact, int8 and the binary scan at
                   every cut (the cut chooses the list form), with the bytes the algorithm needs over that time as a share of
                   the 8 TB/s HBM peak                                                                                        [device]
  recall@k         of the re-scored binary answer against the exact one at every cut and at the default cut, and of the int8
                   answer at its default cut, mean and min over the 32 queries
Medians over ``rounds`` rounds with the min-max spread of the rounds.

  block sweep      one query, cuts 64 / 128 / 256: the whole search and the scan bracket with the scan's workgroups capped at
                   256 / 128 / 64 / 32 / 16 (dewi_b1_tuning_set) — per-wave lists cost the select waves * cut keys per query

    python scripts/bench_binary.py [--n 1048576] [--dim 768] [--ks 10,100] [--batches 1,4] [--iters 50] [--rounds 5]
                                   [--json out.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "oracle"))      # (tests/corpora.py builds its corpora on the oracle's generators)

HBM_PEAK = 8.0e12
CUTS = (128, 256, 512, 1024)


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


def _med(xs):
    return statistics.median(xs), min(xs), max(xs)


def _recall(np, ids, exact_ids, k):
    per = [len(set(ids[j].tolist()) & set(exact_ids[j].tolist())) / k for j in range(ids.shape[0])]
    return [round(float(np.mean(per)), 4), round(float(np.min(per)), 4)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--eta", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import numpy as np
    import torch
    from corpora import embedding_like
    from dewi import _engine as eng

    n, d, eta = a.n, a.dim, a.eta
    X, Q, _, _ = embedding_like(n, d, 3)
    rs = np.random.RandomState(0)
    cols = [rs.rand(n) for _ in range(3)]
    corpus = eng.DeviceCorpus.from_host(X, *cols, "cosine").enable_int8_shadow().enable_binary_shadow()
    del X
    Qd = torch.from_numpy(Q).cuda()
    out = open(a.json, "w") if a.json else None
    bits_bytes = corpus.b1_bits.numel() * 4
    print(f"corpus {n} x {d} fp32 embedding_like ({corpus.corpus_bytes()} B) + int8 copy ({corpus.i8_codes.numel() + 4 * n} B) "
          f"+ binary copy ({bits_bytes} B); eta {eta}")
    set_bits = float(np.unpackbits(corpus.b1_bits[:4096].cpu().numpy().view(np.uint8)).mean())
    print(f"share of 1 bits in the first 4096 rows: {set_bits:.3f}")

    # the binarise pass alone: n * d * 4 bytes read, n * d / 8 written
    for _ in range(3):
        corpus._binarize()
    ms = _events(torch, corpus._binarize, 10)
    print(f"dewi_binarize_rows_f32 (with its output allocation): {ms:.4f} ms, {(n * d * 4 + bits_bytes) / (ms * 1e-3) / 1e12:.3f} TB/s "
          f"= {(n * d * 4 + bits_bytes) / (ms * 1e-3) / HBM_PEAK:.3f} of the 8 TB/s peak   [device]")

    # how many workgroups should a pass with per-wave lists have?  (one query, k = 10)
    lib = corpus._lib
    q1 = Qd[:1].contiguous()
    ids1 = torch.empty((1, 10), dtype=torch.int64, device="cuda")
    sc1 = torch.empty((1, 10), dtype=torch.float32, device="cuda")
    print("\nblock sweep, one query, k 10: cut, workgroups, whole search ms (min - max of the rounds), scan bracket ms   [device]")
    for c in (64, 128, 256):
        for mb in (256, 128, 64, 32, 16):
            assert lib.dewi_b1_tuning_set(mb) == 0
            corpus.drop_cached_workspaces()
            fn = lambda: corpus.search_binary_device(q1, 10, eta, 0.0, c, True, ids1, sc1)
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = _med([_events(torch, fn, a.iters) for _ in range(a.rounds)])
            ms, _ = _scan_ms(torch, eng, fn, a.iters)
            print(f"  cut {c:4d}  blocks {mb:3d}  search {med:8.4f} ({lo:.4f} - {hi:.4f})  scan {ms:8.4f}")
            if out:
                out.write(json.dumps({"case": "block_sweep", "cut": c, "max_blocks": mb, "search_ms": round(med, 5),
                                      "spread_ms": [round(lo, 5), round(hi, 5)], "scan_ms": round(ms, 5)}) + "\n")
    assert lib.dewi_b1_tuning_set(0) == 0
    corpus.drop_cached_workspaces()

    for k in (int(x) for x in a.ks.split(",")):
        exact_ids, _ = corpus.search_device(Qd, k, 0.0, 0.0)
        exact_ids = exact_ids.cpu().numpy()
        recall = {}
        for c in CUTS:
            ids, _ = corpus.search_binary_device(Qd, k, 0.0, 0.0, candidates=c)
            recall[f"binary_{c}"] = _recall(np, ids.cpu().numpy(), exact_ids, k)
        ids, _ = corpus.search_binary_device(Qd, k, 0.0, 0.0)
        recall[f"binary_default_{eng.binary_cut(k, None, n)}"] = _recall(np, ids.cpu().numpy(), exact_ids, k)
        ids, _ = corpus.search_binary_device(Qd, k, 0.0, 0.0, candidates=1024, rescore=False)
        recall["binary_1024_no_rescore"] = _recall(np, ids.cpu().numpy(), exact_ids, k)
        ids, _ = corpus.search_approx_device(Qd, k, 0.0, 0.0)
        recall[f"int8_{2 * k}"] = _recall(np, ids.cpu().numpy(), exact_ids, k)
        print(f"\nk {k}: recall@{k} vs the exact search over {Qd.shape[0]} queries (mean, min): {recall}")

        for b in (int(x) for x in a.batches.split(",")):
            q = Qd[:b].contiguous()
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            sc = torch.empty((b, k), dtype=torch.float32, device="cuda")
            routes = {"exact": lambda: corpus.search_device(q, k, eta, 0.0, ids, sc),
                      "int8": lambda: corpus.search_approx_device(q, k, eta, 0.0, None, True, ids, sc)}
            for c in CUTS:
                routes[f"binary_{c}"] = lambda c=c: corpus.search_binary_device(q, k, eta, 0.0, c, True, ids, sc)
            for _ in range(a.warmup):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            r = {key: [] for key in routes}
            for _ in range(a.rounds):
                for key, fn in routes.items():
                    r[key].append(_events(torch, fn, a.iters))
            rec = {"case": "binary", "k": k, "batch": b, "n": n, "dim": d, "iters": a.iters, "rounds": a.rounds, "recall": recall,
                   "exact_scan_kernel": corpus.scan_kernel_name(b, k)}
            print(f"\nk {k}, batch {b} (exact scan kernel: {rec['exact_scan_kernel']})")
            for key in routes:
                med, lo, hi = _med(r[key])
                print(f"  {key:<14} {med:9.4f} ms   ({lo:.4f} - {hi:.4f})   [device, whole search]")
                rec[key + "_ms"] = round(med, 5)
                rec[key + "_spread_ms"] = [round(lo, 5), round(hi, 5)]
            # the scan kernels alone, with their roofline line (one bracket spans every corpus pass of a call)
            per_pass = {"exact": n * d * 4, "int8": n * (d + 4)}
            per_pass.update({f"binary_{c}": n * d // 8 for c in CUTS})
            for key, row_bytes in per_pass.items():
                ms, launches = _scan_ms(torch, eng, routes[key], a.iters)
                rec[key + "_scan_ms"] = round(ms, 5)
                line = f"  {key:<14} scan bracket {ms:9.4f} ms over {launches} calls"
                passes = 1 if b in (1, 4) and key != "exact" else (1 if b == 1 else None)
                if passes is not None and ms > 0:
                    nbytes = passes * (row_bytes + b * d * 4)
                    rate = nbytes / (ms * 1e-3)
                    rec[key + "_scan_bytes"] = nbytes
                    rec[key + "_scan_share_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
                    line += f"   {nbytes} B, {rate / 1e12:.3f} TB/s algorithmic = {rate / HBM_PEAK:.3f} of the 8 TB/s peak"
                print(line)
            if out:
                out.write(json.dumps(rec) + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()

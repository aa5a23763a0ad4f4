"""Near-duplicate GROUPS at 1 M x 768 fp32 with a bf16 shadow: DeviceCorpus.duplicate_groups_device against
DeviceCorpus.near_duplicates_device (the pairs; its code is the parent commit's, untouched) on the same corpus and threshold in
one process, and the union / finish kernels' own time.

Corpus (seed 0, the recipe of scripts/bench_range_shadow.py): isotropic normalised gaussian rows — nothing in it reaches 0.9 by
chance — then `--planted` rows overwritten by copies of `--planted` other rows (groups of 2) and `--cluster` rows overwritten
by copies of ONE row (one group of `--cluster` + 1, i.e. cluster * (cluster + 1) / 2 pairs).  Threshold 0.9.

Every figure is a median over `rounds` rounds (min - max in brackets), pairs and groups alternating round by round:
  pairs    near_duplicates_device(0.9), wall clock of one run (it synchronises once per chunk)                          [host]
  groups   duplicate_groups_device(0.9, keep="dewi"), the same                                                          [host]
  kernels  the chunks' result lists are collected once and kept; then begin + one dewi_groups_union_lists per chunk, and
           dewi_groups_finish, each between two events                                                                 [device]

    python scripts/bench_groups.py [--n 1048576] [--dim 768] [--rounds 5] [--planted 1000] [--cluster 200] [--json out.jsonl]
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))
sys.path.insert(0, str(REPO / "tests"))


def _fmt(xs, unit="s"):
    return f"{statistics.median(xs):10.4f} {unit}   ({min(xs):.4f} - {max(xs):.4f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--planted", type=int, default=1000)
    ap.add_argument("--cluster", type=int, default=200)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dewi import _engine as eng
    from dewi import _native as nat
    import groups_model as gm

    n, d, thr = a.n, a.dim, a.threshold
    gen = torch.Generator(device="cuda").manual_seed(0)
    emb = torch.empty(n, d, dtype=torch.float32, device="cuda")
    for s in range(0, n, 1 << 16):
        m = min(1 << 16, n - s)
        blk = torch.randn(m, d, generator=gen, device="cuda")
        emb[s:s + m] = blk / torch.linalg.vector_norm(blk, dim=1, keepdim=True)
    perm = torch.randperm(n, generator=gen, device="cuda")
    p, c = a.planted, a.cluster
    emb[perm[:p]] = emb[perm[p:2 * p]]
    emb[perm[2 * p:2 * p + c]] = emb[perm[2 * p + c]].clone()
    dewi32 = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
    ent32 = torch.rand(n, generator=gen, device="cuda", dtype=torch.float32)
    corpus = eng.DeviceCorpus(emb, dewi32, ent32, "cosine").enable_bf16_shadow()
    lib = corpus._lib
    out = open(a.json, "w") if a.json else None

    def emit(rec):
        print(json.dumps(rec))
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, res

    print(f"corpus {n} x {d} fp32 + bf16 shadow, threshold {thr}, {p} planted copies, one cluster of {c} + 1")
    # warm-up of both (workspaces, first launches), and the check: the groups are the components of the pairs
    (pa, pb, _) = corpus.near_duplicates_device(thr)
    (labels, sizes, reps), n_groups = corpus.duplicate_groups_device(thr, keep="dewi")
    want = gm.groups(n, pa.cpu().numpy(), pb.cpu().numpy(), keep="dewi", key=dewi32.cpu().numpy())
    assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(sizes.cpu().numpy(), want[1])
    assert np.array_equal(reps.cpu().numpy(), want[2]) and n_groups == want[3]
    n_pairs = int(pa.shape[0])
    print(f"{n_pairs} pairs, {n_groups} groups, largest {int(sizes.max())}; groups equal the model on the pairs")

    t_pairs, t_groups = [], []
    for _ in range(a.rounds):
        t_pairs.append(wall(lambda: corpus.near_duplicates_device(thr))[0])
        t_groups.append(wall(lambda: corpus.duplicate_groups_device(thr, keep="dewi"))[0])
    print(f"  pairs   near_duplicates_device     {_fmt(t_pairs)}")
    print(f"  groups  duplicate_groups_device    {_fmt(t_groups)}")

    # the kernels' own time: the same chunks' lists, kept, then only the groups entry points between events
    chunks = []
    for s in range(0, n - 1, 2048):
        e = min(n, s + 2048)
        lims, rows, _, _, _ = corpus._range_rows(emb[s:e], thr, 0.0, 0.0, None, None, True, first_row=s)
        if rows.shape[0]:
            chunks.append((s, e - s, lims, rows))
    results = sum(int(ch[3].shape[0]) for ch in chunks)
    ws = torch.empty(int(lib.dewi_groups_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    outs = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3)]
    ng, bad = ctypes.c_int64(0), ctypes.c_int64(0)
    t_union, t_finish = [], []
    for _ in range(a.rounds + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        nat.check(lib.dewi_groups_begin(n, nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        for s, nb, lims, rows in chunks:
            nat.check(lib.dewi_groups_union_lists(n, nat.ptr(lims), nat.ptr(rows), nb, int(rows.shape[0]), s, nat.ptr(ws), ws.numel(),
                                                  nat.stream_ptr()))
        ev[1].record()
        ev[2].record()
        nat.check(lib.dewi_groups_finish(n, 1, nat.ptr(dewi32), 0, nat.ptr(outs[0]), nat.ptr(outs[1]), nat.ptr(outs[2]),
                                         ctypes.byref(ng), ctypes.byref(bad), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        ev[3].record()
        torch.cuda.synchronize()
        t_union.append(ev[0].elapsed_time(ev[1]))
        t_finish.append(ev[2].elapsed_time(ev[3]))
    assert ng.value == n_groups and bad.value == 0 and torch.equal(outs[0], labels)
    t_union, t_finish = t_union[1:], t_finish[1:]          # (the first round is the warm-up)
    print(f"  begin + {len(chunks)} union_lists calls ({results} results)   {_fmt(t_union, 'ms')}")
    print(f"  finish (2 kernels + read-back)     {_fmt(t_finish, 'ms')}")
    emit({"case": "duplicate_groups", "n": n, "dim": d, "threshold": thr, "planted": p, "cluster": c, "pairs": n_pairs,
          "groups": n_groups, "pairs_seconds": round(statistics.median(t_pairs), 4),
          "pairs_spread_seconds": [round(min(t_pairs), 4), round(max(t_pairs), 4)],
          "groups_seconds": round(statistics.median(t_groups), 4),
          "groups_spread_seconds": [round(min(t_groups), 4), round(max(t_groups), 4)],
          "union_calls": len(chunks), "union_results": results, "union_ms": round(statistics.median(t_union), 4),
          "union_spread_ms": [round(min(t_union), 4), round(max(t_union), 4)], "finish_ms": round(statistics.median(t_finish), 4),
          "finish_spread_ms": [round(min(t_finish), 4), round(max(t_finish), 4)]})
    if out:
        out.close()


if __name__ == "__main__":
    main()

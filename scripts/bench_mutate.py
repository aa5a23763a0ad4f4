"""In-place removal and upsert at 1 M x 768 fp32 with a bf16 shadow (`ExactIndex(batch_shadow=True)`): the time of a whole
call, host clock around the call and a device synchronisation, against the only route the parent commit has for the same
change — a fresh `add_batch_columns` + `build` of the resulting corpus — alternating in one process.

The corpus is ingested device-resident (normalised gaussian rows, three payload columns as CUDA tensors).  Per count m
(default 1, 1 000 and 100 000 documents), `rounds` rounds of:
  remove          index.remove(m random ids)                                                      [call + synchronise]
  upsert append   index.upsert_batch(the same m ids, new rows, Payload objects): m new rows        [call + synchronise]
                  (which also brings the index back to its size for the next round)
  upsert replace  index.upsert_batch(m random existing ids, new rows, Payload objects)            [call + synchronise]
  upsert columns  index.upsert_batch_columns(m existing ids, CUDA rows, CUDA columns)             [call + synchronise]
  rebuild         ExactIndex + add_batch_columns(the raw matrix, resident on the device) + build: normalise, payload
                  columns, shadow — the parent's cheapest route (its time does not depend on m)  [call + synchronise]
and once per run `rebuild from host`: the same with the raw matrix in host memory (the upload included), `host_rounds` times.
Medians over the rounds with their min-max spread.  `moved GB/s`: the bytes the mutation must move, 2 * m * (row bytes of
matrix + shadow + two payload floats), over the call time.

    python scripts/bench_mutate.py [--n 1048576] [--dim 768] [--counts 1,1000,100000] [--rounds 5] [--host-rounds 2]
                                   [--json out.jsonl]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _med(xs):
    return statistics.median(xs), min(xs), max(xs)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--counts", default="1,1000,100000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import numpy as np
    import torch
    from dewi.backends import ExactIndex
    from dewi.types import Payload

    n, d = a.n, a.dim
    gen = torch.Generator(device="cuda").manual_seed(0)
    raw = torch.empty(n, d, dtype=torch.float32, device="cuda")
    for s in range(0, n, 1 << 16):
        raw[s:s + (1 << 16)] = torch.randn(min(1 << 16, n - s), d, generator=gen, device="cuda")
    cols = {name: torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) for name in ("dewi", "ht_mean", "hi_mean")}
    ids = [f"doc_{i:08d}" for i in range(n)]
    row_bytes = d * 4 + d * 2 + 8

    def build_fresh(block, columns, copy=False):
        # copy=False: a device block is adopted and normalised in place, the cheapest the route gets (the block stays a valid
        # raw matrix for the next round: normalised rows are raw rows too)
        f = ExactIndex(d, "cosine", batch_shadow=True)
        f.add_batch_columns(ids, block, columns, copy=copy)
        f.build()
        return f

    index = build_fresh(raw, cols, copy=True)                     # the index under test owns its matrix
    index.rows_of(ids[:1])                                        # the id -> row map is made once, outside the timings
    rs = np.random.RandomState(1)
    out = open(a.json, "w") if a.json else None
    print(f"corpus {n} x {d} fp32 + bf16 shadow, device-resident ingest; row bytes (matrix + shadow + payload) {row_bytes}")

    def report(rec, key, label, times, moved=None):
        med, lo, hi = _med(times)
        rec[key + "_ms"] = round(med, 4)
        rec[key + "_spread_ms"] = [round(lo, 4), round(hi, 4)]
        extra = ""
        if moved is not None:
            rec[key + "_moved_gbps"] = round(moved / (med * 1e-3) / 1e9, 3)
            extra = f"   {rec[key + '_moved_gbps']:9.3f} GB/s of the {moved} bytes it must move"
        print(f"  {label:<34} {med:11.4f} ms   ({lo:.4f} - {hi:.4f}){extra}")

    for m in (int(x) for x in a.counts.split(",")):
        new_rows = rs.standard_normal((m, d)).astype(np.float32)
        pays = [Payload(dewi=float(v), ht_mean=float(v) / 2, hi_mean=float(v) / 3) for v in rs.rand(m)]
        new_dev = torch.from_numpy(new_rows).cuda()
        cols_dev = {name: torch.rand(m, generator=gen, device="cuda", dtype=torch.float64) for name in cols}
        t = {"remove": [], "append": [], "replace": [], "columns": [], "rebuild": []}
        for r in range(a.rounds + 1):                             # round 0 warms every shape up and is dropped
            cur = index._doc_ids
            gone = [cur[i] for i in rs.choice(len(cur), m, replace=False).tolist()]
            gone_set = set(gone)
            some = [cur[i] for i in rs.choice(len(cur), 2 * m + 8, replace=False).tolist() if cur[i] not in gone_set][:m]
            step = [_timed(torch, lambda: index.remove(gone)),
                    _timed(torch, lambda: index.upsert_batch(gone, new_rows, pays)),
                    _timed(torch, lambda: index.upsert_batch(some, new_rows[: len(some)], pays[: len(some)])),
                    _timed(torch, lambda: index.upsert_batch_columns(some, new_dev[: len(some)],
                                                                     {k: v[: len(some)] for k, v in cols_dev.items()})),
                    _timed(torch, lambda: build_fresh(raw, cols))]
            assert len(index._doc_ids) == n
            if r:
                for key, v in zip(t, step):
                    t[key].append(v)
        moved = 2 * m * row_bytes
        rec = {"case": "mutate", "m": m, "n": n, "dim": d, "rounds": a.rounds, "moved_bytes": moved}
        print(f"\nm = {m}")
        report(rec, "remove", "remove", t["remove"], moved)
        report(rec, "append", "upsert_batch, m new ids", t["append"], moved)
        report(rec, "replace", "upsert_batch, m existing ids", t["replace"], moved)
        report(rec, "columns", "upsert_batch_columns, device", t["columns"], moved)
        report(rec, "rebuild", "add_batch_columns + build (device)", t["rebuild"])
        rec["rebuild_over_remove"] = round(rec["rebuild_ms"] / rec["remove_ms"], 2)
        rec["rebuild_over_replace"] = round(rec["rebuild_ms"] / rec["replace_ms"], 2)
        print(f"  rebuild / remove = x{rec['rebuild_over_remove']}, rebuild / upsert(existing) = x{rec['rebuild_over_replace']}")
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    if a.host_rounds > 0:
        host = raw.cpu().numpy()
        host_cols = {name: c.cpu().numpy() for name, c in cols.items()}
        times = [_timed(torch, lambda: build_fresh(host, host_cols)) for _ in range(a.host_rounds + 1)][1:]
        rec = {"case": "rebuild_from_host", "n": n, "dim": d, "rounds": a.host_rounds, "upload_bytes": n * d * 4}
        print("\nthe raw matrix in host memory")
        report(rec, "rebuild_host", "add_batch_columns + build (host)", times)
        if out:
            out.write(json.dumps(rec) + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()

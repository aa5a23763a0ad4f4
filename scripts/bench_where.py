"""Metadata predicates at 1 M x 768 fp32 with three attribute columns (year int32, site categorical, noise fp32).

Nothing here sets a pass mark: the numbers are recorded (results.jsonl and a README.md with the table in --out).

  (a) the mask kernel alone: `dewi_predicate_masks` called back to back on one stream with arguments packed once, device
      events around at least 200 launches; reported per launch with the bytes it moves (4 bytes per row and column read,
      1 byte per row and program written) and that rate's share of the HBM peak.  One predicate and 32 predicates per call.
  (b) `make_filter_where` end to end (mask kernel + dewi_filter_prepare + the count's synchronisation) at selectivities of
      about 1 %, 10 % and 50 %, against the path the index had before: the same predicate evaluated with NumPy on host
      columns and passed to `make_filter(mask)` (N-byte upload included) — same process, the two alternating.
  (c) 32 per-query predicates: `make_query_filters_where` against NumPy masks [32, N] + `make_query_filters`.
  (d) one `search(filter=where)` against `search(filter=<the prepared filter>)`: what preparing on the fly costs.

    python scripts/bench_where.py [--n 1048576] [--dim 768] [--launches 200] [--reps 9] [--out profiles/r21/where]
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

HBM_PEAK = 8.0e12          # bytes / s, the MI355X's specified HBM3E bandwidth
N_SITES = 3000


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r21" / "where"))
    a = ap.parse_args()
    if a.launches < 200:
        raise SystemExit("--launches: at least 200")

    import numpy as np
    import torch
    from dewi import _native as nat
    from dewi.backends import ExactIndex
    from dewi.where import col, compile_programs

    lib = nat.load_library()
    torch.cuda.set_device(0)
    n, d = a.n, a.dim
    rs = np.random.RandomState(0)
    torch.manual_seed(0)
    emb = torch.randn(n, d, dtype=torch.float32, device="cuda")
    index = ExactIndex(dim=d)
    index.add_batch_columns([f"doc_{i:07d}" for i in range(n)], emb, {"dewi": torch.rand(n, dtype=torch.float64, device="cuda")})
    index.build()
    sites = [f"site{j:04d}.org" for j in range(N_SITES)]
    site_code = rs.randint(0, N_SITES, n).astype(np.int32)
    year = rs.randint(1990, 2026, n).astype(np.int32)
    noise = rs.rand(n).astype(np.float32)
    # the categorical column is set from its strings once (host work a user does once per corpus, not per predicate)
    index.set_attributes(year=year, site=np.asarray(sites, dtype=object)[site_code].tolist(), noise=noise)
    corpus = index._corpus
    Q = np.random.RandomState(1).randn(1, d).astype(np.float32)

    def predicate(first_year, n_sites, max_noise):
        chosen = [sites[j] for j in rs.choice(N_SITES, n_sites, replace=False)]
        where = (col("year") >= first_year) & col("site").isin(chosen) & (col("noise") < max_noise)
        member = np.zeros(N_SITES, dtype=bool)
        member[[int(s[4:8]) for s in chosen]] = True

        def host_mask():
            return (year >= first_year) & member[site_code] & (noise < np.float32(max_noise))
        return where, host_mask

    cases = {"1%": predicate(2017, 300, 0.4), "10%": predicate(2008, 1200, 0.5), "50%": predicate(1990, 2400, 0.625)}
    records = []

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    def alternate(new, old, reps):
        """Median wall milliseconds of two paths run alternately (one warm-up each)."""
        new(), old()
        t_new, t_old = [], []
        for _ in range(reps):
            t_new.append(wall(new)[0])
            t_old.append(wall(old)[0])
        return statistics.median(t_new), statistics.median(t_old), min(t_new), min(t_old)

    # ---- (a) the kernel alone
    for n_programs in (1, 32):
        ws = [cases["10%"][0]] * n_programs
        prog = compile_programs(ws, index)
        cols = [index._attr_columns()[name].view() for name in prog.columns]
        ptrs = (ctypes.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
        types = (ctypes.c_int32 * len(cols))(*[1 if c.dtype == torch.float32 else 0 for c in cols])
        flat = [i for p in prog.programs for i in p]
        instr = (nat.PredInstr * len(flat))(*[nat.PredInstr(*i) for i in flat])
        lens = (ctypes.c_int32 * n_programs)(*[len(p) for p in prog.programs])
        sets = torch.from_numpy(prog.sets.view(np.int32)).cuda()
        out = torch.empty((n_programs, n), dtype=torch.uint8, device="cuda")
        stream = nat.stream_ptr()

        def launch():
            nat.check(lib.dewi_predicate_masks(ptrs, types, len(cols), n, instr, lens, n_programs, sets.data_ptr(), sets.numel(),
                                               None, out.data_ptr(), stream))
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            launch()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.launches
        instr_per_launch = sum(len(p) for p in prog.programs)
        n_launches = -(-n_programs // min(32, max(1, 272 // len(prog.programs[0]))))
        moved = n_launches * len(cols) * 4 * n + n_programs * n
        records.append({"part": "a", "programs": n_programs, "instructions": instr_per_launch, "kernel_launches_per_call": n_launches,
                        "calls_timed": a.launches, "ms_per_call": ms, "bytes_moved": moved, "GBps": moved / ms / 1e6,
                        "share_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK})

    # ---- (b) make_filter_where end to end against NumPy + make_filter
    for name, (where, host_mask) in cases.items():
        f = index.make_filter_where(where)
        m = host_mask()
        assert len(f) == int(m.sum()) and np.array_equal(f.byte_mask().cpu().numpy().astype(bool), m), name
        dev, host, dev_min, host_min = alternate(lambda: index.make_filter_where(where), lambda: index.make_filter(host_mask()), a.reps)
        numpy_only = statistics.median([_timeit(host_mask) for _ in range(a.reps)])
        records.append({"part": "b", "selectivity": name, "allowed": len(f), "where_ms": dev, "numpy_make_filter_ms": host,
                        "where_min_ms": dev_min, "numpy_make_filter_min_ms": host_min, "numpy_mask_alone_ms": numpy_only})

    # ---- (c) 32 per-query predicates
    per_query = [predicate(1990 + (j % 30), 300 + 60 * j, 0.3 + 0.02 * j) for j in range(32)]
    ws = [p[0] for p in per_query]
    qf = index.make_query_filters_where(ws)
    masks = np.stack([p[1]() for p in per_query])
    assert qf.n_allowed.tolist() == masks.sum(axis=1).tolist()
    dev, host, dev_min, host_min = alternate(lambda: index.make_query_filters_where(ws),
                                             lambda: index.make_query_filters(np.stack([p[1]() for p in per_query])), max(3, a.reps // 3))
    records.append({"part": "c", "queries": 32, "union": qf.n_union, "where_ms": dev, "numpy_make_query_filters_ms": host,
                    "where_min_ms": dev_min, "numpy_make_query_filters_min_ms": host_min})

    # ---- (d) search with a predicate prepared on the fly against a prepared filter
    for name, (where, _) in cases.items():
        f = index.make_filter_where(where)
        fly, prepared, fly_min, prepared_min = alternate(lambda: index.search_batch(Q, a.k, 0.3, 0.0, filter=where),
                                                         lambda: index.search_batch(Q, a.k, 0.3, 0.0, filter=f), 2 * a.reps)
        records.append({"part": "d", "selectivity": name, "search_where_ms": fly, "search_prepared_ms": prepared,
                        "search_where_min_ms": fly_min, "search_prepared_min_ms": prepared_min})

    out_dir = Path(a.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "results.jsonl", "w") as fh:
        for r in records:
            r.update(n=n, dim=d)
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))
    (out_dir / "README.md").write_text(table(records, n, d, a))


def _timeit(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def table(records, n, d, a) -> str:
    lines = [f"# Metadata predicates, {n} x {d} fp32, three attribute columns", "",
             "Written by `scripts/bench_where.py`; milliseconds, medians (minimum in brackets) of alternating runs in one process.", "",
             "## (a) `dewi_predicate_masks` alone", "",
             f"Device events around {a.launches} back-to-back calls, arguments packed once; bytes = 4 per row and column read per kernel "
             "launch + 1 per row and program written.", "",
             "| programs per call | instructions | kernel launches per call | ms per call | MB moved | GB/s | share of the 8 TB/s HBM peak |",
             "|---|---|---|---|---|---|---|"]
    for r in (r for r in records if r["part"] == "a"):
        lines.append(f"| {r['programs']} | {r['instructions']} | {r['kernel_launches_per_call']} | {r['ms_per_call']:.4f} | "
                     f"{r['bytes_moved'] / 1e6:.1f} | {r['GBps']:.0f} | {100 * r['share_of_hbm_peak']:.1f} % |")
    lines += ["", "## (b) `make_filter_where` against NumPy on host columns + `make_filter(mask)`", "",
              "| selectivity | rows allowed | make_filter_where | NumPy + make_filter | of which NumPy alone | speed-up |", "|---|---|---|---|---|---|"]
    for r in (r for r in records if r["part"] == "b"):
        lines.append(f"| {r['selectivity']} | {r['allowed']} | {r['where_ms']:.3f} ({r['where_min_ms']:.3f}) | "
                     f"{r['numpy_make_filter_ms']:.3f} ({r['numpy_make_filter_min_ms']:.3f}) | {r['numpy_mask_alone_ms']:.3f} | "
                     f"{r['numpy_make_filter_ms'] / r['where_ms']:.1f}x |")
    lines += ["", "## (c) 32 per-query predicates", "",
              "| union rows | make_query_filters_where | NumPy masks + make_query_filters | speed-up |", "|---|---|---|---|"]
    for r in (r for r in records if r["part"] == "c"):
        lines.append(f"| {r['union']} | {r['where_ms']:.2f} ({r['where_min_ms']:.2f}) | {r['numpy_make_query_filters_ms']:.2f} "
                     f"({r['numpy_make_query_filters_min_ms']:.2f}) | {r['numpy_make_query_filters_ms'] / r['where_ms']:.1f}x |")
    lines += ["", "## (d) one search: the predicate prepared on the fly against a prepared filter", "",
              "| selectivity | search(filter=where) | search(filter=prepared) | on-the-fly cost |", "|---|---|---|---|"]
    for r in (r for r in records if r["part"] == "d"):
        lines.append(f"| {r['selectivity']} | {r['search_where_ms']:.3f} ({r['search_where_min_ms']:.3f}) | {r['search_prepared_ms']:.3f} "
                     f"({r['search_prepared_min_ms']:.3f}) | {r['search_where_ms'] - r['search_prepared_ms']:.3f} |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()

"""Facets at 1 M rows: `dewi_facet_run` and `index.facet` next to the way a histogram is made today on the device,
`torch.bincount(col[mask] - lo, minlength=...)`.

Nothing here sets a pass mark: the numbers are recorded (results.jsonl and a README.md with the tables in --out).  Every case is
timed between device events around --launches back-to-back calls after a warm-up, in one process, the two forms one after the
other; "whole call" rows are host wall time around a call that ends in a synchronisation (medians of alternating runs).

  (a) a 1000-value categorical column over all rows;
  (b) the same under a `Where` at about 1 %, 10 % and 50 %: the whole call (`index.facet(filter=where)`, mask kernel and host
      copy included) and the facet call alone over a prepared mask;
  (c) 32 predicates in one call against 32 calls;
  (d) with value statistics (count / min / max / sum of an fp32 column) against bincount + scatter_reduce;
  (e) the one-bin (fully contended) column against the uniform column, on both paths;
  (f) 2^20 bins on path 1 (global counters);
  (g) `facet_range` for 32 queries against `range_search_batch` + `np.bincount` on the host.

Bytes moved by the facet pass: per launch 4 per row (key) + 4 per row with values + 1 per row and selection; its share of
the 8 TB/s HBM peak is those bytes over the time of the WHOLE call (clearing and finishing launches included).

    python scripts/bench_facets.py [--n 1048576] [--dim 64] [--launches 200] [--reps 9] [--out profiles/r24/facets]
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
N_SITES = 1000


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(REPO / "profiles" / "r24" / "facets"))
    a = ap.parse_args()

    import numpy as np
    import torch
    from dewi import _native as nat
    from dewi.backends import ExactIndex
    from dewi.where import col

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
    index.set_attributes(site=np.asarray(sites, dtype=object)[site_code].tolist(), year=rs.randint(1990, 2026, n).astype(np.int32),
                         noise=rs.rand(n).astype(np.float32), one=np.full(n, 7, dtype=np.int32),
                         wide=rs.randint(0, 1 << 20, n).astype(np.int32))
    corpus = index._corpus
    have = index._attr_columns()
    site, noise, one, wide = (have[x].view() for x in ("site", "noise", "one", "wide"))
    records = []

    def events(fn):
        """Milliseconds per call: device events around a.launches back-to-back calls, after 20 warm-up calls."""
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def alternate(new, old, reps):
        new(), old()
        t_new, t_old = [], []
        for _ in range(reps):
            t_new.append(wall(new))
            t_old.append(wall(old))
        return statistics.median(t_new), statistics.median(t_old)

    def facet_call(keys, n_bins, masks=None, values=None, key_lo=0):
        """A closure that enqueues one `dewi_facet_run` with everything packed once -> (fn, counts, stats)."""
        p = 1 if masks is None else int(masks.shape[0])
        vt = 0 if values is None else (2 if values.dtype == torch.float32 else 1)
        slots = p * (n_bins + 2)
        need = int(lib.dewi_facet_workspace_bytes(n_bins, p, vt))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        counts = torch.empty(slots, dtype=torch.int64, device="cuda")
        st = None
        if vt:
            st = [torch.empty(slots, dtype=torch.int64, device="cuda"), torch.empty(slots, dtype=values.dtype, device="cuda"),
                  torch.empty(slots, dtype=values.dtype, device="cuda"),
                  torch.empty(slots, dtype=torch.float64 if vt == 2 else torch.int64, device="cuda")]
        stream = nat.stream_ptr()
        args = (keys.data_ptr(), 0, n, key_lo, None, n_bins, 0 if masks is None else 1, p, None if masks is None else masks.data_ptr(),
                None, None, 0, None if values is None else values.data_ptr(), vt, counts.data_ptr(),
                *([t.data_ptr() for t in st] if st else [None] * 4), ws.data_ptr(), need, stream)

        def fn():
            nat.check(lib.dewi_facet_run(*args))
        return fn, counts.view(p, n_bins + 2), st

    def rec(case, form, ms, moved=None, **extra):
        r = {"case": case, "form": form, "ms": ms, **extra}
        if moved is not None:
            r.update(bytes_moved=moved, GBps=moved / ms / 1e6, share_of_hbm_peak=moved / (ms * 1e-3) / HBM_PEAK)
        records.append(r)
        print(json.dumps(r), flush=True)

    def plan(n_bins, sel, p, vt):
        return nat.facet_plan(n, 0, n_bins, sel, p, vt)

    # ---- (a) all rows
    fn, counts, _ = facet_call(site, N_SITES)
    fn()
    want = torch.bincount(site, minlength=N_SITES)
    assert torch.equal(counts[0, :N_SITES], want) and int(counts[0, N_SITES:].sum()) == 0
    rec("a: 1000 values, all rows", "dewi_facet_run", events(fn), 4 * n, plan=plan(N_SITES, 0, 1, 0))
    rec("a: 1000 values, all rows", "torch.bincount", events(lambda: torch.bincount(site, minlength=N_SITES)))

    # ---- (b) under a predicate
    for name, where in (("1%", col("noise") < 0.01), ("10%", col("noise") < 0.1), ("50%", col("noise") < 0.5)):
        masks = index._where_masks([where])
        mb = masks[0].view(torch.bool)
        fn, counts, _ = facet_call(site, N_SITES, masks=masks)
        fn()
        assert torch.equal(counts[0, :N_SITES], torch.bincount(site[mb], minlength=N_SITES))
        rec(f"b: under a Where at {name}, facet call alone", "dewi_facet_run", events(fn), 5 * n, selected=int(mb.sum()))
        rec(f"b: under a Where at {name}, facet call alone", "torch.bincount(col[mask])", events(lambda: torch.bincount(site[mb], minlength=N_SITES)))
        new, old = alternate(lambda: index.facet("site", filter=where),
                             lambda: torch.bincount(site[index._where_masks([where])[0].view(torch.bool)], minlength=N_SITES).cpu(), a.reps)
        rec(f"b: under a Where at {name}, whole call", "index.facet(filter=where)", new)
        rec(f"b: under a Where at {name}, whole call", "where mask + torch.bincount + copy", old)

    # ---- (c) 32 predicates
    wheres = [col("noise") < 0.02 * (j + 1) for j in range(32)]
    masks = index._where_masks(wheres)
    fn, counts, _ = facet_call(site, N_SITES, masks=masks)
    fn()
    singles = [facet_call(site, N_SITES, masks=masks[j: j + 1])[0] for j in range(32)]
    assert torch.equal(counts[31, :N_SITES], torch.bincount(site[masks[31].view(torch.bool)], minlength=N_SITES))
    pl = plan(N_SITES, 1, 32, 0)
    rec("c: 32 predicates", "one dewi_facet_run", events(fn), pl["launches"] * 4 * n + 32 * n, plan=pl)
    rec("c: 32 predicates", "32 dewi_facet_run", events(lambda: [f() for f in singles]), 32 * 5 * n)
    rec("c: 32 predicates", "32 torch.bincount(col[mask])",
        events(lambda: [torch.bincount(site[masks[j].view(torch.bool)], minlength=N_SITES) for j in range(32)]))

    # ---- (d) value statistics
    fn, counts, st = facet_call(site, N_SITES, values=noise)
    fn()
    idx = site.to(torch.int64)

    def torch_stats():
        c = torch.bincount(site, minlength=N_SITES)
        s = torch.bincount(site, weights=noise.double(), minlength=N_SITES)
        lo = torch.full((N_SITES,), float("inf"), device="cuda").scatter_reduce_(0, idx, noise, "amin")
        hi = torch.full((N_SITES,), float("-inf"), device="cuda").scatter_reduce_(0, idx, noise, "amax")
        return c, s, lo, hi
    c, s, lo, hi = torch_stats()
    torch.cuda.synchronize()
    assert torch.equal(st[0][:N_SITES], c) and torch.equal(st[1][:N_SITES], lo) and torch.equal(st[2][:N_SITES], hi)
    assert float((st[3][:N_SITES] - s).abs().max()) < 1e-9
    rec("d: with value statistics", "dewi_facet_run", events(fn), 8 * n, plan=plan(N_SITES, 0, 1, 2))
    rec("d: with value statistics", "torch bincount x2 + scatter_reduce x2", events(torch_stats))

    # ---- (e) contention: one bin against uniform, both paths
    for force, label in ((-1, "path 0 (LDS)"), (1, "path 1 (global)")):
        lib.dewi_facet_tuning_set(force, 0)
        for keys, what in ((site, "uniform column"), (one, "one-bin column")):
            for values, vl in ((None, ""), (noise, " with values")):
                fn, counts, _ = facet_call(keys, N_SITES, values=values)
                fn()
                torch.cuda.synchronize()
                assert int(counts.sum()) == n
                rec(f"e: {what}{vl}", f"dewi_facet_run, {label}", events(fn), (4 if values is None else 8) * n)
        lib.dewi_facet_tuning_set(-1, 0)
    rec("e: one-bin column", "torch.bincount", events(lambda: torch.bincount(one, minlength=N_SITES)))

    # ---- (f) 2^20 bins, path 1
    fn, counts, _ = facet_call(wide, 1 << 20)
    fn()
    assert torch.equal(counts[0, :1 << 20], torch.bincount(wide, minlength=1 << 20))
    pl = plan(1 << 20, 0, 1, 0)
    assert pl["path"] == 1
    rec("f: 2^20 bins", "dewi_facet_run (path 1)", events(fn), 4 * n + 8 * (1 << 20), plan=pl)
    rec("f: 2^20 bins", "torch.bincount", events(lambda: torch.bincount(wide, minlength=1 << 20)))

    # ---- (g) facet_range for 32 queries
    Q = emb[rs.randint(0, n, 32)].cpu().numpy() + 0.5 * rs.randn(32, d).astype(np.float32)
    thr = 0.35
    code_host = site.cpu().numpy()

    def host_form():
        lims, rows, _, _ = index.range_search_batch(Q, thr, sort=False)
        return [np.bincount(code_host[rows[lims[j]: lims[j + 1]]], minlength=N_SITES) for j in range(32)], int(lims[-1])
    want, t_rows = host_form()
    got = index.facet_range(Q, thr, "site")
    assert all(g.counts.tolist() == w.tolist() for g, w in zip(got, want))
    new, old = alternate(lambda: index.facet_range(Q, thr, "site"), host_form, a.reps)
    rec("g: facet_range, 32 queries", "index.facet_range", new, rows_in_range=t_rows)
    rec("g: facet_range, 32 queries", "range_search_batch + np.bincount", old, rows_in_range=t_rows)

    out_dir = Path(a.out)
    out_dir.mkdir(parents=True, exist_ok=True)
    with open(out_dir / "results.jsonl", "w") as fh:
        for r in records:
            r.update(n=n, dim=d)
            fh.write(json.dumps(r) + "\n")
    (out_dir / "README.md").write_text(table(records, n, a))


def table(records, n, a) -> str:
    lines = [f"# Facets, {n} rows", "",
             f"Written by `scripts/bench_facets.py`; milliseconds per call.  Device events around {a.launches} back-to-back calls "
             "(`dewi_facet_run`, `torch` rows) or median host wall time of alternating runs (`index.*` rows and what they are compared "
             "with).  GB/s: the bytes the facet pass has to read (and, for 2^20 bins, the counters it clears) over the time of the "
             "whole call; share of the 8 TB/s HBM peak likewise.", "",
             "| case | form | ms per call | MB | GB/s | share of HBM peak |", "|---|---|---|---|---|---|"]
    for r in records:
        moved = r.get("bytes_moved")
        lines.append(f"| {r['case']} | {r['form']} | {r['ms']:.4f} | " +
                     (f"{moved / 1e6:.1f} | {r['GBps']:.0f} | {100 * r['share_of_hbm_peak']:.1f} % |" if moved else "| | |"))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()

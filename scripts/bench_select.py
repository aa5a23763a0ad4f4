"""Subset selection at 1 M x 768 fp32: the time of one pick (one ``dewi_select_run`` pass over the corpus) against the
one-query ``search_device`` step of the same corpus, in one process, the two alternating round by round (device events,
medians of ``--rounds`` rounds with the min-max spread).

The corpus is made on the device after the recipe of tests/corpora.py::embedding_like — ``unit(centre[label] + noise randn +
shift sqrt(dim) u)``, 48 gaussian centres, cluster sizes skewed — with every ``--copy-every``-th row a near-copy (noise 1e-3) of
its predecessor; the relevance is uniform in [0, 1).

Reported per case: ms per pick (a run of ``--budget`` picks between two events, divided by the picks made), the algorithmic
bytes of a pass over ALL rows (rows x (row bytes + 12 B of state)) over that time as a share of the 8 TB/s HBM peak, the ratio
to the search step, and the rows still live after the run (with ``max_sim`` a pass reads only those: the share of peak is then
an upper bound on the bytes, a lower bound on nothing — read the ratio).  Cases: fp32 and bf16 at ``--dim``, fp32 at
``--dim`` / 2, each without a cut and with ``max_sim = 0.9``; then whole calls of ``--long`` picks.

    python scripts/bench_select.py [--n 1048576] [--dim 768] [--budget 256] [--long 1000,10000] [--json out.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))

HBM_PEAK = 8.0e12


def make_rows(torch, n, dim, gen, copy_every, chunk=65536):
    centres = torch.randn((48, dim), device="cuda", generator=gen)
    u = torch.randn(dim, device="cuda", generator=gen)
    u /= u.norm()
    sizes = torch.distributions.Dirichlet(torch.full((48,), 0.3)).sample()
    labels = torch.sort(torch.multinomial(sizes, n, replacement=True, generator=None)).values.cuda()
    out = torch.empty((n, dim), device="cuda")
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        x = centres[labels[a:b]] + 0.6 * torch.randn((b - a, dim), device="cuda", generator=gen) + 1.5 * dim ** 0.5 * u
        out[a:b] = x / x.norm(dim=1, keepdim=True)
    if copy_every > 0:
        src = out[0::copy_every][: out[1::copy_every].shape[0]]
        x = src + 1e-3 / dim ** 0.5 * torch.randn(src.shape, device="cuda", generator=gen)
        out[1::copy_every] = x / x.norm(dim=1, keepdim=True)
    return out


def timed(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--budget", type=int, default=256)
    ap.add_argument("--long", default="1000,10000")
    ap.add_argument("--copy-every", type=int, default=10)
    ap.add_argument("--search-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="also write one JSON line per case here")
    a = ap.parse_args()

    import torch
    from dewi import _engine as eng

    torch.manual_seed(5)
    gen = torch.Generator(device="cuda").manual_seed(11)
    n = a.n
    out = open(a.json, "w") if a.json else None
    print(f"{n} rows, every {a.copy_every}th a near-copy; {a.rounds} rounds; a run of {a.budget} picks per round")

    def case(name, corpus, max_sim, budget, rounds, with_search=True):
        d, elem_bytes = corpus.dim, 2 if corpus.is_bf16 else 4
        q = corpus.emb[12345 % n].float().reshape(1, -1).contiguous()
        ids = torch.empty((1, 10), dtype=torch.int64, device="cuda")
        sc = torch.empty((1, 10), dtype=torch.float32, device="cuda")
        state = {}

        def select():
            state["out"] = corpus.select_subset_device(budget, 0.5, max_sim)

        def search():
            for _ in range(a.search_iters):
                corpus.search_device(q, 10, 0.3, 0.0, ids, sc)

        select()
        search()
        torch.cuda.synchronize()
        t_sel, t_scan = [], []
        for _ in range(rounds):
            t_sel.append(timed(torch, select))
            if with_search:
                t_scan.append(timed(torch, search) / a.search_iters)
        kk = int(state["out"][2].item())
        ws = corpus.cached_workspaces()[("select", n)]
        n64 = (n + 63) // 64 * 64
        live = n - int(ws[4096 + 256 + 8 * n64: 4096 + 256 + 8 * n64 + n].sum().item())
        per_pick = statistics.median(t_sel) / max(kk, 1)
        bytes_all = n * (d * elem_bytes + 12)
        rec = {"case": name, "n": n, "dim": d, "elem_bytes": elem_bytes, "max_sim": max_sim, "budget": budget, "picked": kk,
               "call_ms": round(statistics.median(t_sel), 3), "call_spread_ms": [round(min(t_sel), 3), round(max(t_sel), 3)],
               "ms_per_pick": round(per_pick, 5), "share_of_hbm_peak_on_all_rows": round(bytes_all / (per_pick * 1e-3) / HBM_PEAK, 4),
               "rows_live_after": live}
        line = (f"  {name:<28} {kk:6d} picks  {rec['call_ms']:10.3f} ms/call  {per_pick:8.4f} ms/pick  "
                f"{rec['share_of_hbm_peak_on_all_rows']:.3f} of peak (all rows)  {live} rows live after")
        if with_search:
            scan = statistics.median(t_scan)
            rec.update(search_step_ms=round(scan, 5), search_step_spread_ms=[round(min(t_scan), 5), round(max(t_scan), 5)],
                       search_kernel=corpus.scan_kernel_name(1, 10), pick_over_search_step=round(per_pick / scan, 3))
            line += f"  search step {scan:.4f} ms  x{per_pick / scan:.3f}"
        print(line, flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    rows = make_rows(torch, n, a.dim, gen, a.copy_every)
    rel = torch.rand(n, device="cuda", generator=gen)
    f32 = eng.DeviceCorpus(rows, rel, torch.zeros(n, device="cuda"))
    for max_sim in (None, 0.9):
        case(f"fp32 {a.dim} max_sim {max_sim}", f32, max_sim, a.budget, a.rounds)
    for b in [int(x) for x in a.long.split(",") if x]:
        case(f"fp32 {a.dim} whole call of {b}", f32, None, b, 1, with_search=False)
        case(f"fp32 {a.dim} whole call of {b}, 0.9", f32, 0.9, b, 1, with_search=False)
    bf16 = eng.DeviceCorpus(rows.to(torch.bfloat16), rel, torch.zeros(n, device="cuda"))
    for max_sim in (None, 0.9):
        case(f"bf16 {a.dim} max_sim {max_sim}", bf16, max_sim, a.budget, a.rounds)
    del bf16, f32, rows
    half = a.dim // 2
    rows = make_rows(torch, n, half, gen, a.copy_every)
    f32h = eng.DeviceCorpus(rows, rel, torch.zeros(n, device="cuda"))
    for max_sim in (None, 0.9):
        case(f"fp32 {half} max_sim {max_sim}", f32h, max_sim, a.budget, a.rounds)
    if out:
        out.close()


if __name__ == "__main__":
    main()

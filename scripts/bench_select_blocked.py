"""The blocked subset selection against the one-pick form, measured in one process on bench_select.py's corpus (1 M x 768 fp32
``embedding_like`` rows, every 10th a near-copy; also bf16 768 and fp32 384).  Device events, medians of ``--reps`` with the
min-max spread; the one-pick form is the yardstick of every figure and runs in the same script.

Parts (``--parts``, comma separated):
  apply   one apply pass with p picks (``dewi_select_seed_blocked`` with p seeds in one pass: the pass and nothing else) for
          p = 1 / 4 / 8 / 16 / 32 / block_max, against one one-pick launch (``dewi_select_seed`` with one seed)
  seeds   ``--seeds`` seeds through ``dewi_select_seed`` and through ``dewi_select_seed_blocked`` (block 32)
  calls   whole calls of ``--budgets`` picks at lambda 0.5, without a cut and with max_sim 0.9, one-pick and block 8 / 16 / 32:
          time, rounds, passes, picks per pass.  ``--one-pick-reps`` repetitions for the one-pick calls (a call of 100 000
          picks takes most of a minute)
  trace   ONE blocked call (budget 1000, block 32) and nothing else: run it under ``rocprofv3 --kernel-trace --stats`` to read
          the round kernel's, the key pass' and the apply pass' times on their own

``--nan-row R`` makes row R all NaN (live, eligible, never given a pen: every blocked round takes one pick) — with small
``--budgets`` the two cases where the blocked form is expected to be the slower one.

    python scripts/bench_select_blocked.py [--corpus fp32|bf16|fp32half] [--parts apply,seeds,calls] [--budgets 1000,10000]
                                           [--nan-row R] [--out-dir profiles/r18/select_blocked] [--tag NAME]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "dewi-design-for-an-entropy-weighted-index-for-text-image-corpora_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--corpus", default="fp32", choices=["fp32", "bf16", "fp32half"])
    ap.add_argument("--parts", default="apply,seeds,calls")
    ap.add_argument("--budgets", default="1000,10000")
    ap.add_argument("--blocks", default="8,16,32")
    ap.add_argument("--seeds", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one-pick-reps", type=int, default=5)
    ap.add_argument("--copy-every", type=int, default=10)
    ap.add_argument("--nan-row", type=int, default=-1, help="make this row all NaN: a live row that never gets a pen, so every "
                                                            "round of the blocked form takes one pick")
    ap.add_argument("--out-dir", default=None, help="write NAME.txt and NAME.jsonl here (NAME: --tag)")
    ap.add_argument("--tag", default=None)
    a = ap.parse_args()

    import torch
    from bench_select import make_rows, timed
    from dewi import _engine as eng
    from dewi import _native as nat

    torch.manual_seed(5)
    gen = torch.Generator(device="cuda").manual_seed(11)
    n = a.n
    dim = a.dim // 2 if a.corpus == "fp32half" else a.dim
    rows = make_rows(torch, n, dim, gen, a.copy_every)
    rel = torch.rand(n, device="cuda", generator=gen)
    if a.nan_row >= 0:
        rows[a.nan_row] = float("nan")
        rel[a.nan_row] = 0.0          # (a NaN row is penalty-free: with a relevance like the others' it is picked early and gone)
    if a.corpus == "bf16":
        rows = rows.to(torch.bfloat16)
    corpus = eng.DeviceCorpus(rows, rel, torch.zeros(n, device="cuda"))
    lib, elem = corpus._lib, corpus._elem
    bmax = int(lib.dewi_select_block_max(dim, elem))
    tag = a.tag or f"{a.corpus}_{dim}"
    txt = jsonl = None
    if a.out_dir:
        Path(a.out_dir).mkdir(parents=True, exist_ok=True)
        txt, jsonl = open(Path(a.out_dir) / f"{tag}.txt", "w"), open(Path(a.out_dir) / f"{tag}.jsonl", "w")

    def emit(line, rec):
        print(line, flush=True)
        if txt:
            txt.write(line + "\n")
            txt.flush()
            jsonl.write(json.dumps(dict(rec, corpus=a.corpus, n=n, dim=dim)) + "\n")
            jsonl.flush()

    def med(ts):
        return round(statistics.median(ts), 4), [round(min(ts), 4), round(max(ts), 4)]

    emit(f"# {n} x {dim} {a.corpus}, every {a.copy_every}th row a near-copy" + (f", row {a.nan_row} all NaN" if a.nan_row >= 0 else "")
         + f"; block_max {bmax}; medians of {a.reps} (min .. max)", {"case": "header", "block_max": bmax, "reps": a.reps, "nan_row": a.nan_row})
    parts = a.parts.split(",")
    need = int(lib.dewi_select_blocked_workspace_bytes(n, dim, elem, bmax))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stream = nat.stream_ptr()
    seed_rows = torch.randint(0, n, (max(a.seeds, 64),), device="cuda", generator=gen, dtype=torch.int64)
    INF = float("inf")

    def begin():
        nat.check(lib.dewi_select_begin(n, dim, elem, None, nat.ptr(ws), need, stream))

    if "apply" in parts:
        def one_pick():
            nat.check(lib.dewi_select_seed(nat.ptr(rows), elem, n, dim, nat.ptr(seed_rows), 1, INF, nat.ptr(ws), need, stream))
        begin()
        one_pick()
        torch.cuda.synchronize()
        base, spread = med([timed(torch, one_pick) for _ in range(a.reps)])
        emit(f"one-pick launch (dewi_select_seed, 1 seed)          {base:9.4f} ms  {spread}", {"case": "apply", "picks": 1, "form": "one-pick",
                                                                                                "ms": base, "spread_ms": spread})
        for p in sorted({p for p in (1, 4, 8, 16, 32, bmax) if p <= bmax}):
            def blocked(p=p):
                nat.check(lib.dewi_select_seed_blocked(nat.ptr(rows), elem, n, dim, nat.ptr(seed_rows), p, INF, nat.ptr(ws), need, stream, p))
            begin()
            blocked()
            torch.cuda.synchronize()
            t, spread = med([timed(torch, blocked) for _ in range(a.reps)])
            emit(f"apply pass with {p:3d} picks                          {t:9.4f} ms  {spread}  = {t / p:.4f} ms/pick, "
                 f"x{base * p / t:.2f} against {p} one-pick launches",
                 {"case": "apply", "picks": p, "form": "blocked", "ms": t, "spread_ms": spread, "ms_per_pick": round(t / p, 5),
                  "speedup_over_one_pick": round(base * p / t, 3)})

    if "seeds" in parts:
        k = a.seeds
        def seeds_one():
            begin()
            nat.check(lib.dewi_select_seed(nat.ptr(rows), elem, n, dim, nat.ptr(seed_rows), k, INF, nat.ptr(ws), need, stream))
        def seeds_blocked():
            begin()
            nat.check(lib.dewi_select_seed_blocked(nat.ptr(rows), elem, n, dim, nat.ptr(seed_rows), k, INF, nat.ptr(ws), need, stream,
                                                   min(32, bmax)))
        t1, s1 = med([timed(torch, seeds_one) for _ in range(a.one_pick_reps)])
        seeds_blocked()
        tb, sb = med([timed(torch, seeds_blocked) for _ in range(a.reps)])
        emit(f"{k} seeds: dewi_select_seed {t1:.2f} ms {s1}; dewi_select_seed_blocked (block {min(32, bmax)}) {tb:.2f} ms {sb}: x{t1 / tb:.2f}",
             {"case": "seeds", "seeds": k, "one_pick_ms": t1, "one_pick_spread_ms": s1, "blocked_ms": tb, "blocked_spread_ms": sb,
              "block": min(32, bmax), "speedup": round(t1 / tb, 3)})

    if "calls" in parts:
        for budget in [int(x) for x in a.budgets.split(",") if x]:
            for max_sim in (None, 0.9):
                state = {}
                def call(ppp):
                    state["out"] = corpus.select_subset_device(budget, 0.5, max_sim, picks_per_pass=ppp, return_stats=True)
                call(None)
                torch.cuda.synchronize()
                t1, s1 = med([timed(torch, lambda: call(None)) for _ in range(a.one_pick_reps)])
                want = state["out"][0].clone()
                kk = int(state["out"][2].item())
                emit(f"budget {budget} max_sim {max_sim}: one-pick  {t1:10.2f} ms {s1}  {kk} picks",
                     {"case": "call", "budget": budget, "max_sim": max_sim, "form": "one-pick", "ms": t1, "spread_ms": s1, "picked": kk,
                      "reps": a.one_pick_reps})
                for block in [int(x) for x in a.blocks.split(",") if x and int(x) <= bmax]:
                    call(block)
                    tb, sb = med([timed(torch, lambda: call(block)) for _ in range(a.reps)])
                    st = state["out"][-1]
                    same = bool(torch.equal(state["out"][0], want))
                    emit(f"budget {budget} max_sim {max_sim}: block {block:2d}  {tb:10.2f} ms {sb}  x{t1 / tb:.2f}  {st['rounds']} rounds, "
                         f"{st['passes']} passes, {kk / max(st['passes'], 1):.1f} picks/pass  same rows: {same}",
                         {"case": "call", "budget": budget, "max_sim": max_sim, "form": "blocked", "block": block, "ms": tb,
                          "spread_ms": sb, "speedup": round(t1 / tb, 3), "rounds": st["rounds"], "passes": st["passes"],
                          "picked": kk, "same_rows_as_one_pick": same})

    if "trace" in parts:
        out = corpus.select_subset_device(1000, 0.5, None, picks_per_pass=min(32, bmax), return_stats=True)
        torch.cuda.synchronize()
        emit(f"trace case: 1000 picks, block {min(32, bmax)}: {out[-1]}", {"case": "trace", "stats": out[-1]})
    if txt:
        txt.close()
        jsonl.close()


if __name__ == "__main__":
    main()

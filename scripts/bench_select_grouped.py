"""Subset selection with group quotas against the ungrouped selection, measured in one process on bench_select.py's corpus
(1 M x 768 fp32 ``embedding_like`` rows, every 10th a near-copy; also bf16).  Device events; the variants are interleaved
(every repetition runs each of them once), ``--reps`` repetitions, median with the min-max spread.

Variants, each in the one-pick form and in the blocked form (``--block``), ``--budget`` picks at lambda 0.5, no max_sim:
  a  ungrouped: ``select_subset_device`` as it was (the same numbers taken on the parent commit go beside these)
  b  grouped, quotas that never bind: labels row % ``--groups``, per_group = budget — the cost of the feature where it does
     nothing: the label read of the opening pass and what a grouped launch adds
  c  grouped, labels row % ``--groups``, per_group ``--per-group``: groups fill, their rows are struck out
Parts (``--parts``): ``calls`` the six whole calls; ``open`` a run of ONE pick, ungrouped and grouped (the opening key pass, one
pick launch and the closing launch: where a grouped run's fixed extra cost sits); ``curve`` variant c in ``--chunks`` resumed
runs of budget / chunks picks each: how the time per pick falls as groups fill (ungrouped beside it).

    python scripts/bench_select_grouped.py [--corpus fp32|bf16] [--parts calls,open,curve] [--out-dir profiles/r19/select_grouped]
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
    ap.add_argument("--corpus", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--parts", default="calls,open,curve")
    ap.add_argument("--budget", type=int, default=10000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--block", type=int, default=32)
    ap.add_argument("--chunks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--copy-every", type=int, default=10)
    ap.add_argument("--out-dir", default=None, help="write NAME.txt and NAME.jsonl here (NAME: --tag)")
    ap.add_argument("--tag", default=None)
    a = ap.parse_args()

    import torch
    from bench_select import make_rows, timed
    from dewi import _engine as eng
    from dewi import _native as nat

    torch.manual_seed(5)
    gen = torch.Generator(device="cuda").manual_seed(11)
    n, dim, budget = a.n, a.dim, a.budget
    rows = make_rows(torch, n, dim, gen, a.copy_every)          # bench_select_blocked.py's corpus and relevance, draw for draw
    rel = torch.rand(n, device="cuda", generator=gen)
    if a.corpus == "bf16":
        rows = rows.to(torch.bfloat16)
    corpus = eng.DeviceCorpus(rows, rel, torch.zeros(n, device="cuda"))
    lib, elem = corpus._lib, corpus._elem
    block = min(a.block, int(lib.dewi_select_block_max(dim, elem)))
    labels = (torch.arange(n, device="cuda") % a.groups).to(torch.int32)
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
        return round(statistics.median(ts), 3), [round(min(ts), 3), round(max(ts), 3)]

    emit(f"# {n} x {dim} {a.corpus}, every {a.copy_every}th row a near-copy; budget {budget}, {a.groups} groups (row % {a.groups}), "
         f"block {block}; {a.reps} interleaved repetitions, median (min .. max)",
         {"case": "header", "budget": budget, "groups": a.groups, "per_group": a.per_group, "block": block, "reps": a.reps})
    parts = a.parts.split(",")
    grouped = {"b": dict(group_labels=labels, n_groups=a.groups, per_group=budget),
               "c": dict(group_labels=labels, n_groups=a.groups, per_group=a.per_group)}

    if "calls" in parts:
        variants = [(v, ppp) for v in ("a", "b", "c") for ppp in (None, block)]
        out, times = {}, {k: [] for k in variants}

        def call(v, ppp):
            out[(v, ppp)] = corpus.select_subset_device(budget, 0.5, None, picks_per_pass=ppp, return_stats=True, **grouped.get(v, {}))
        for k in variants:                                     # warm-up: the workspace, the kernels' first launches
            corpus.select_subset_device(64, 0.5, None, picks_per_pass=k[1], **grouped.get(k[0], {}))
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k in variants:
                times[k].append(timed(torch, lambda: call(*k)))
        base = {}
        for k in variants:
            t, spread = med(times[k])
            kk = int(out[k][2].item())
            st = out[k][-1]
            form = "one-pick" if k[1] is None else f"block {k[1]}"
            base.setdefault(k[1], (t, spread))
            t0, s0 = base[k[1]]
            same = bool(torch.equal(out[k][0], out[(k[0], None)][0]))
            emit(f"{k[0]} {form:9s} {t:10.2f} ms {spread}  {kk} picks, {st['passes']} passes, {t / max(kk, 1):.4f} ms/pick"
                 f"  against a: {t - t0:+.2f} ms (a's spread {s0[1] - s0[0]:.2f} ms)  rows as the one-pick form: {same}",
                 {"case": "call", "variant": k[0], "form": form, "ms": t, "spread_ms": spread, "picked": kk, "passes": st["passes"],
                  "rounds": st["rounds"], "ms_per_pick": round(t / max(kk, 1), 5), "minus_a_ms": round(t - t0, 3),
                  "a_spread_ms": round(s0[1] - s0[0], 3), "same_rows_as_one_pick": same})
        assert torch.equal(out[("a", None)][0], out[("b", None)][0]), "quotas that never bind changed the selection"

    if "open" in parts:
        times = {"a": [], "b": []}
        for _ in range(a.reps + 1):
            for v in ("a", "b"):
                times[v].append(timed(torch, lambda: corpus.select_subset_device(1, 0.5, None, **grouped.get(v, {}))))
        for v in ("a", "b"):
            t, spread = med(times[v][1:])                                  # (the first round warms up)
            emit(f"one pick, {'ungrouped' if v == 'a' else 'grouped  '}: begin + opening key pass + one pick launch"
                 f"{' + groups_begin + closing launch' if v == 'b' else ''}  {t:8.3f} ms {spread}",
                 {"case": "open", "variant": v, "ms": t, "spread_ms": spread})

    if "curve" in parts:
        stream = nat.stream_ptr()
        need = int(lib.dewi_select_grouped_workspace_bytes(n, dim, elem, a.groups, block))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        o_rows = torch.empty(budget, dtype=torch.int64, device="cuda")
        o_gain = torch.empty(budget, dtype=torch.float32, device="cuda")
        o_cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        step = budget // a.chunks
        for v in ("a", "c"):
            grp = () if v == "a" else (nat.ptr(labels), a.groups, None, a.per_group, None)
            run = lib.dewi_select_run if v == "a" else lib.dewi_select_run_grouped
            per_chunk = [[] for _ in range(a.chunks)]
            for _ in range(a.reps):
                nat.check(lib.dewi_select_begin(n, dim, elem, None, nat.ptr(ws), need, stream))
                nat.check(lib.dewi_select_groups_begin(n, dim, elem, a.groups, nat.ptr(ws), need, stream))
                for c in range(a.chunks):
                    per_chunk[c].append(timed(torch, lambda: nat.check(run(
                        nat.ptr(rows), elem, n, dim, nat.ptr(rel), step, 0.5, float("inf"), 0, nat.ptr(o_rows), nat.ptr(o_gain),
                        nat.ptr(o_cnt), None, None, nat.ptr(ws), need, stream, *grp))))
            for c in range(a.chunks):
                t, spread = med(per_chunk[c])
                emit(f"{v} one-pick, picks {c * step:6d} .. {(c + 1) * step:6d}: {t:9.2f} ms {spread}  {t / step:.4f} ms/pick",
                     {"case": "curve", "variant": v, "chunk": c, "picks": step, "ms": t, "spread_ms": spread,
                      "ms_per_pick": round(t / step, 5)})
    if txt:
        txt.close()
        jsonl.close()


if __name__ == "__main__":
    main()

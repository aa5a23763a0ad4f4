"""Compare the device code of two builds function by function.

Each directory holds `<unit>.s` files made with
    hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S <unit>.hip -o <dir>/<unit>.s
(the Makefile's flags).  Every function of BEFORE must exist in AFTER with the same instructions; basic-block numbers and
assembler comments are ignored (they shift when a unit gains functions).  Functions only AFTER has are counted, not compared.

    python scripts/compare_kernel_asm.py [--reordered-ok PREFIX ...] BEFORE_DIR AFTER_DIR knn_scan knn_scan_any_f32 ...

For every function that differs the script prints its figures on both sides: instruction count, whether the multiset of
mnemonics is the same, and .vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size from the
unit's kernel metadata.  --reordered-ok PREFIX (repeatable) accepts a differing function whose name (the mangled name
without its `_ZN4dewi<len>` head) starts with PREFIX when all of these figures are equal: the same instructions in another
order or with other register names.  Every other difference fails.
"""
import argparse
import re
import sys
from collections import Counter
from pathlib import Path

FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def functions(path: Path) -> dict:
    out, cur, body = {}, None, []
    for line in path.read_text().splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m and cur is None:
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        code = line.split(";")[0].rstrip()
        if code:
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
    return out


def metadata(path: Path) -> dict:
    """Kernel name -> {figure: value} from the amdhsa.kernels list of a unit's .s file."""
    out, cur, inside = {}, None, False
    for line in path.read_text().splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line and not line.startswith(" "):   # next top-level key: the list is over
            break
        if line.startswith("  - "):
            cur = {}
        m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\S+)$", line)
        if m and cur is not None:
            if m.group(1) == ".name":
                out[m.group(2)] = cur
            elif m.group(1) in FIGURES:
                cur[m.group(1)] = int(m.group(2))
    return out


def instructions(body: list) -> list:
    """Mnemonics of a function body: labels and assembler directives left out."""
    return [c.split()[0] for c in body if not c.endswith(":") and not c.lstrip().startswith(".")]


def short_name(mangled: str) -> str:
    m = re.match(r"^_ZN\d+dewi\d+", mangled)
    return mangled[m.end():] if m else mangled


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reordered-ok", action="append", default=[], metavar="PREFIX")
    ap.add_argument("before", type=Path)
    ap.add_argument("after", type=Path)
    ap.add_argument("units", nargs="+")
    args = ap.parse_args()
    total = same = reordered = 0
    bad, notes = [], []
    for unit in args.units:
        a, b = functions(args.before / f"{unit}.s"), functions(args.after / f"{unit}.s")
        ma, mb = metadata(args.before / f"{unit}.s"), metadata(args.after / f"{unit}.s")
        unit_same = 0
        for name, body in a.items():
            total += 1
            if b.get(name) == body:
                unit_same += 1
                continue
            if name not in b:
                bad.append((unit, name, "missing"))
                continue
            ia, ib = instructions(body), instructions(b[name])
            fa, fb = ma.get(name, {}), mb.get(name, {})
            same_set = Counter(ia) == Counter(ib)
            weak = len(ia) == len(ib) and same_set and fa == fb and len(fa) == len(FIGURES)
            figures = " ".join(f"{k[1:]}={fa.get(k)}/{fb.get(k)}" for k in FIGURES)
            line = f"{unit} {name}: instructions={len(ia)}/{len(ib)} mnemonics={'same' if same_set else 'DIFFERENT'} {figures}"
            if weak and any(short_name(name).startswith(p) for p in args.reordered_ok):
                reordered += 1
                notes.append(line)
            else:
                bad.append((unit, name, "differs"))
                notes.append(line + "   <-- FAILS")
        same += unit_same
        print(f"{unit}: {len(a)} functions before, {len(b)} after ({len(set(b) - set(a))} new); identical: {unit_same} of {len(a)}")
    print(f"identical: {same} of {total}; accepted as reordered: {reordered}; failing: {len(bad)}")
    if notes:
        print("functions that differ (before/after):")
        for line in notes:
            print(f"  {line}")
    for unit, name, why in bad:
        if why == "missing":
            print(f"  missing: {unit} {name}")
    return 0 if not bad else 1


if __name__ == "__main__":
    sys.exit(main())

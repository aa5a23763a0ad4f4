"""Compare the device code of two builds function by function.

Each directory holds `<unit>.s` files made with
    hipcc -O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S <unit>.hip -o <dir>/<unit>.s
(the Makefile's flags).  Every function of BEFORE must exist in AFTER with the same instructions; basic-block numbers and
assembler comments are ignored (they shift when a unit gains functions).  Functions only AFTER has are counted, not compared.

    python scripts/compare_kernel_asm.py BEFORE_DIR AFTER_DIR knn_scan knn_scan_any_f32 ...
"""
import re
import sys
from pathlib import Path


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


def main() -> int:
    before, after, units = Path(sys.argv[1]), Path(sys.argv[2]), sys.argv[3:]
    total = same = 0
    bad = []
    for unit in units:
        a, b = functions(before / f"{unit}.s"), functions(after / f"{unit}.s")
        for name, body in a.items():
            total += 1
            if b.get(name) == body:
                same += 1
            else:
                bad.append((unit, name, "missing" if name not in b else "differs"))
        print(f"{unit}: {len(a)} functions before, {len(b)} after ({len(set(b) - set(a))} new)")
    print(f"identical: {same} of {total}")
    for unit, name, why in bad[:20]:
        print(f"  {why}: {unit} {name}")
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())

"""Choose the corpus seeds of tests/test_hip_select.py part C on the CPU: for every case the lowest seed from 1 on at which the
float64 model ALONE decides at least three quarters of the picks before its first undecided one.  Prints the SEEDS_C table
(the cases whose seed is not 1) and every case's decided count.  No GPU is needed or used."""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "tests")]

import test_hip_select as t  # noqa: E402


def main():
    table = {}
    for n, dim, budget, clustered, lam, max_sim in t.CASES_C:
        for seed in range(1, 50):
            *_, rows, _, decided = t.float64_model(n, dim, budget, clustered, lam, max_sim, seed)
            ok = len(rows) == budget and 4 * decided >= 3 * budget
            print(f"{n} x {dim} {'clustered' if clustered else 'plain'} lambda {lam} max_sim {max_sim} seed {seed}: "
                  f"{len(rows)} picks, {decided} decided{'' if ok else '  (rejected)'}", flush=True)
            if ok:
                if seed != 1:
                    table[(n, dim, clustered, lam, max_sim)] = seed
                break
        else:
            raise SystemExit("no seed below 50 serves this case")
    print("SEEDS_C =", table)


if __name__ == "__main__":
    main()

"""A NumPy/Python model of in-place removal and upsert: the row order rule, stated independently of the package.

Removal of a set D of m rows from n (n' = n - m): rows are not shifted down, the tail fills the holes.  The holes H are the
members of D below n', ascending; the movers M are the rows of [n', n) that are not in D, ascending; |H| = |M|; row M[i] moves
to slot H[i]; then the corpus is cut to n' rows.  Upsert: a known id keeps its row, new ids are appended in call order.

Everything here is a plain loop over rows, on purpose: the package plans a removal by sorting the deleted rows, so the two
share no code and no idea.  tests/test_mutate_model_host.py pins the model itself with hand-written examples.
"""
from typing import Dict, Hashable, List, Sequence, Tuple

import numpy as np


def remove_pairs(n: int, deleted) -> Tuple[List[int], List[int], int]:
    """-> (movers M, holes H, n'): row M[i] moves to slot H[i]."""
    dele = set(int(r) for r in deleted)
    assert all(0 <= r < n for r in dele)
    n_keep = n - len(dele)
    holes = [r for r in range(n_keep) if r in dele]
    movers = [r for r in range(n_keep, n) if r not in dele]
    assert len(holes) == len(movers)
    return movers, holes, n_keep


def remove_order(n: int, deleted) -> np.ndarray:
    """int64 [n']: the OLD row that sits at each new row after the removal."""
    movers, holes, n_keep = remove_pairs(n, deleted)
    order = list(range(n_keep))
    for m, h in zip(movers, holes):
        order[h] = m
    return np.asarray(order, dtype=np.int64)


def remove_ids(ids: Sequence[Hashable], deleted_ids) -> List[Hashable]:
    """The id list after removing ``deleted_ids`` (every one present exactly once)."""
    where = {d: i for i, d in enumerate(ids)}
    assert len(where) == len(ids)
    return [ids[i] for i in remove_order(len(ids), [where[d] for d in deleted_ids]).tolist()]


def upsert_rows(ids: Sequence[Hashable], upserted: Sequence[Hashable]) -> Tuple[List[int], List[Hashable]]:
    """-> (the row every upserted id is written to, the id list afterwards): a known id keeps its row, new ids take rows
    n, n + 1, ... in call order."""
    out = list(ids)
    where: Dict[Hashable, int] = {d: i for i, d in enumerate(out)}
    rows = []
    for d in upserted:
        if d not in where:
            where[d] = len(out)
            out.append(d)
        rows.append(where[d])
    assert len(set(rows)) == len(rows), "an id twice in one call"
    return rows, out

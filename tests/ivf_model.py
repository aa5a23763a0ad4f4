"""A NumPy model of the two integer stages of the IVF route (csrc/ivf.hip), word for word what include/dewi_hip.h documents.

``lists_model``  what ``dewi_ivf_lists_build`` leaves in its buffer: the offsets, the listed rows, the error word.
``probe_model``  what ``dewi_ivf_probe_prepare`` leaves per group of queries (header, list, query words) and returns (|U|, |F_j|).

Sorting only (stable argsort of one integer key over rows that are ascending already); no loop over bins or rows, so the
cell counts the header allows (65536 cells x 4 buckets) cost milliseconds.  tests/test_ivf_model_host.py checks both against
naive loops; tests/test_hip_ivf_lists.py compares the device buffers with them by exact equality.
"""
from typing import List, NamedTuple, Tuple

import numpy as np

HEADER_WORDS = 16        # kFilterHeaderWords (csrc/scan_common.hpp): the list starts at word 16 of a group's buffer
MAX_BUCKETS = 8          # kFilterMaxBuckets: header[G .. 8] = |U|, header[9] = G


def _valid_rows(assign, n_cells: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rows whose assignment lies in [0, n_cells), their cells), both int64, rows ascending."""
    a = np.asarray(assign).astype(np.int64).ravel()
    rows = np.nonzero((a >= 0) & (a < n_cells))[0].astype(np.int64)
    return rows, a[rows]


def lists_model(assign, n_cells: int, G: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (offsets uint32 [n_cells * G + 1], rows uint32 [n_listed], dropped).

    The rows with 0 <= assign < n_cells ordered by (cell, row % G, row); offsets cell-major / bucket-minor (segment (cell, b)
    is rows[offsets[cell * G + b] : offsets[cell * G + b + 1]]), offsets[-1] = n_listed; dropped = the other rows."""
    rows, cells = _valid_rows(assign, n_cells)
    bins = cells * G + rows % G
    order = np.argsort(bins, kind="stable")                 # rows are ascending: stable keeps them so inside a bin
    offsets = np.zeros(n_cells * G + 1, np.int64)
    np.cumsum(np.bincount(bins, minlength=n_cells * G), out=offsets[1:])
    return offsets.astype(np.uint32), rows[order].astype(np.uint32), int(np.asarray(assign).size - rows.size)


class ProbeGroup(NamedTuple):
    header: np.ndarray      # uint32 [16]
    rows: np.ndarray        # uint32 [|U|]: the list from word 16
    words: np.ndarray       # uint32 [|U|]: the query bits per list position, from word 16 + n_rows


class ProbeModel(NamedTuple):
    groups: List[ProbeGroup]
    n_union: np.ndarray     # int64 [n_groups]
    n_allowed: np.ndarray   # int64 [B]


def probe_model(assign, n_cells: int, G: int, probe_ids, group: int) -> ProbeModel:
    """Per group of ``group`` consecutive queries: bits[cell] = OR of 1 << i over the group's queries i that name the cell
    with a valid id; the union list = rows of cells with bits != 0 ordered by (row % G, cell, row); words[p] = bits[cell of
    the row at p]; header[b] = start of bucket b (b < G), header[G .. 8] = |U|, header[9] = G, header[10 .. 15] = 0.
    |F_j| = the rows of query j's distinct valid cells."""
    ids = np.asarray(probe_ids, dtype=np.int64)
    assert ids.ndim == 2 and 1 <= group <= 32 and 1 <= G <= MAX_BUCKETS
    n_queries = ids.shape[0]
    rows, cells = _valid_rows(assign, n_cells)
    sizes = np.bincount(cells, minlength=n_cells).astype(np.int64)
    valid = (ids >= 0) & (ids < n_cells)

    # |F_j|: a cell counts once per query however often the query names it
    named = np.zeros((n_queries, n_cells), bool)
    q_of, slot = np.nonzero(valid)
    named[q_of, ids[q_of, slot]] = True
    n_allowed = named.astype(np.int64) @ sizes

    groups, n_union = [], []
    for q0 in range(0, n_queries, group):
        sub = named[q0:q0 + group]
        bits = (sub.astype(np.uint64) << np.arange(sub.shape[0], dtype=np.uint64)[:, None]).sum(axis=0).astype(np.uint32)
        take = bits[cells] != 0
        r, c = rows[take], cells[take]
        order = np.argsort((r % G) * n_cells + c, kind="stable")
        r, c = r[order], c[order]
        header = np.zeros(HEADER_WORDS, np.uint32)
        header[1:G + 1] = np.cumsum(np.bincount(r % G, minlength=G))
        header[G:MAX_BUCKETS + 1] = r.size
        header[MAX_BUCKETS + 1] = G
        groups.append(ProbeGroup(header, r.astype(np.uint32), bits[c]))
        n_union.append(r.size)
    return ProbeModel(groups, np.asarray(n_union, np.int64), n_allowed)

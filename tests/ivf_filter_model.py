"""A NumPy model of the IVF probe under a user filter (``dewi_ivf_probe_prepare_filtered``, csrc/ivf.hip), word for word what
include/dewi_hip.h documents: the unfiltered probe of tests/ivf_model.py with every row the user does not allow dropped, the
order kept, and the query words cut down to the queries that allow the row.

Sorting only, as in ivf_model.py.  tests/test_ivf_filter_model_host.py checks it against naive loops;
tests/test_hip_ivf_filtered_lists.py compares the device buffers with it by exact equality.
"""
import numpy as np

from ivf_model import HEADER_WORDS, MAX_BUCKETS, ProbeGroup, ProbeModel, _valid_rows


def probe_filtered_model(assign, n_cells: int, G: int, probe_ids, group: int, allow, per_query: bool) -> ProbeModel:
    """``allow``: bytes (nonzero = allowed), [n_rows] shared by every query or (``per_query``) [n_queries, n_rows].

    Per group of ``group`` consecutive queries q0 .. : bits[cell] as in ``probe_model``; allow(row) = every bit of the group if
    the shared mask allows the row, else 0 — per query: bit i set iff query q0 + i allows it; a row is listed iff
    w = bits[cell(row)] & allow(row) != 0 and its word is w; listed rows ordered by (row % G, cell, row); the header as in
    ``probe_model`` over the listed rows.  n_allowed[j] = the listed rows whose word holds query j's bit."""
    ids = np.asarray(probe_ids, dtype=np.int64)
    assert ids.ndim == 2 and 1 <= group <= 32 and 1 <= G <= MAX_BUCKETS
    n_queries = ids.shape[0]
    n_rows = np.asarray(assign).size
    allow = np.asarray(allow) != 0
    assert allow.shape == ((n_queries, n_rows) if per_query else (n_rows,))
    rows, cells = _valid_rows(assign, n_cells)
    valid = (ids >= 0) & (ids < n_cells)
    named = np.zeros((n_queries, n_cells), bool)
    q_of, slot = np.nonzero(valid)
    named[q_of, ids[q_of, slot]] = True

    groups, n_union = [], []
    n_allowed = np.zeros(n_queries, np.int64)
    for q0 in range(0, n_queries, group):
        sub = named[q0:q0 + group]
        nq = sub.shape[0]
        shifts = np.arange(nq, dtype=np.uint64)[:, None]
        bits = (sub.astype(np.uint64) << shifts).sum(axis=0).astype(np.uint32)
        if per_query:
            ok = (allow[q0:q0 + nq][:, rows].astype(np.uint64) << shifts).sum(axis=0).astype(np.uint32)
        else:
            ok = np.where(allow[rows], np.uint32(0xFFFFFFFF), np.uint32(0))
        w = bits[cells] & ok
        take = w != 0
        r, c, w = rows[take], cells[take], w[take]
        order = np.argsort((r % G) * n_cells + c, kind="stable")
        r, w = r[order], w[order]
        header = np.zeros(HEADER_WORDS, np.uint32)
        header[1:G + 1] = np.cumsum(np.bincount(r % G, minlength=G))
        header[G:MAX_BUCKETS + 1] = r.size
        header[MAX_BUCKETS + 1] = G
        groups.append(ProbeGroup(header, r.astype(np.uint32), w.astype(np.uint32)))
        n_union.append(r.size)
        for i in range(nq):
            n_allowed[q0 + i] = np.count_nonzero((w >> np.uint32(i)) & np.uint32(1))
    return ProbeModel(groups, np.asarray(n_union, np.int64), n_allowed)

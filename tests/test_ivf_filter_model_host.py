"""The NumPy model of the IVF probe under a user filter (tests/ivf_filter_model.py) against naive loops written from
include/dewi_hip.h, on tiny inputs (no GPU).  tests/test_hip_ivf_filtered_lists.py then holds the device buffers to the model
word for word."""
import numpy as np
import pytest

from ivf_filter_model import probe_filtered_model
from ivf_model import probe_model


def _naive(assign, n_cells, G, probe_ids, group, allow, per_query):
    n_queries = len(probe_ids)
    out, n_union, n_allowed = [], [], [0] * n_queries
    for q0 in range(0, n_queries, group):
        mine = probe_ids[q0:q0 + group]
        bits = [0] * n_cells
        for i, ids in enumerate(mine):
            for cell in ids:
                if 0 <= cell < n_cells:
                    bits[cell] |= 1 << i
        rows, words, header = [], [], [0] * 16
        for b in range(G):
            header[b] = len(rows)
            for cell in range(n_cells):
                for row in range(len(assign)):
                    if assign[row] != cell or row % G != b:
                        continue
                    if per_query:
                        ok = sum(1 << i for i in range(len(mine)) if allow[q0 + i][row])
                    else:
                        ok = 0xFFFFFFFF if allow[row] else 0
                    w = bits[cell] & ok
                    if w:
                        rows.append(row)
                        words.append(w)
                        for i in range(len(mine)):
                            n_allowed[q0 + i] += (w >> i) & 1
        for w in range(G, 9):
            header[w] = len(rows)
        header[9] = G
        out.append((header, rows, words))
        n_union.append(len(rows))
    return out, n_union, n_allowed


def _assignments(n, n_cells, seed):
    rs = np.random.RandomState(seed)
    bad = rs.randint(0, n_cells, n).astype(np.int32)
    bad[rs.choice(n, 4, replace=False)] = [-1, n_cells, np.iinfo(np.int32).max, np.iinfo(np.int32).min]
    return {"random": rs.randint(0, n_cells, n).astype(np.int32), "round_robin": (np.arange(n) % n_cells).astype(np.int32),
            "first": np.zeros(n, np.int32), "bad": bad}


def _probes(rs, b, nprobe, n_cells):
    ids = rs.randint(0, n_cells, (b, nprobe)).astype(np.int64)
    ids[rs.rand(b, nprobe) < 0.2] = -1
    ids[rs.rand(b, nprobe) < 0.1] = n_cells
    ids[rs.rand(b, nprobe) < 0.1] = 1 << 40
    ids[b // 2] = -1
    if nprobe > 1:
        ids[0, 1] = ids[0, 0]
    return ids


def _same(m, want, note):
    groups, n_union, n_allowed = want
    assert m.n_union.tolist() == n_union and m.n_allowed.tolist() == n_allowed, note
    assert len(m.groups) == len(groups)
    for got, (header, rows, words) in zip(m.groups, groups):
        assert got.header.dtype == got.rows.dtype == got.words.dtype == np.uint32
        assert got.header.tolist() == header and got.rows.tolist() == rows and got.words.tolist() == words, note


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("group", [1, 3, 8, 32])
def test_filtered_model_is_the_naive_expansion(G, group):
    n, n_cells = 150, 7
    rs = np.random.RandomState(10 * G + group)
    for name, assign in _assignments(n, n_cells, seed=G).items():
        for b, nprobe in ((1, 1), (group + 3, 3), (32, 5)):
            ids = _probes(rs, b, nprobe, n_cells)
            shared = {"half": rs.rand(n) < 0.5, "few": rs.rand(n) < 0.03, "none": np.zeros(n, bool),
                      "bytes": rs.choice(np.array([0, 1, 2, 255], np.uint8), n)}
            for mname, allow in shared.items():
                m = probe_filtered_model(assign, n_cells, G, ids, group, allow, False)
                _same(m, _naive(assign.tolist(), n_cells, G, ids.tolist(), group, (np.asarray(allow) != 0).tolist(), False),
                      (name, mname, b, nprobe))
            per = rs.rand(b, n) < rs.choice([0.0, 0.02, 0.5, 1.0], b)[:, None]
            m = probe_filtered_model(assign, n_cells, G, ids, group, per, True)
            _same(m, _naive(assign.tolist(), n_cells, G, ids.tolist(), group, per.tolist(), True), (name, "per query", b, nprobe))
            assert m.n_allowed[b // 2] == 0


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("group", [1, 8, 32])
def test_all_ones_mask_is_the_unfiltered_probe(G, group):
    n, n_cells = 300, 11
    rs = np.random.RandomState(G + group)
    for name, assign in _assignments(n, n_cells, seed=G + 5).items():
        ids = _probes(rs, 2 * group + 3, 4, n_cells)
        want = probe_model(assign, n_cells, G, ids, group)
        for allow, per_query in ((np.ones(n, np.uint8), False), (np.full(n, 255, np.uint8), False),
                                 (np.ones((ids.shape[0], n), bool), True)):
            got = probe_filtered_model(assign, n_cells, G, ids, group, allow, per_query)
            assert got.n_union.tolist() == want.n_union.tolist() and got.n_allowed.tolist() == want.n_allowed.tolist(), name
            for a, b in zip(got.groups, want.groups):
                assert np.array_equal(a.header, b.header) and np.array_equal(a.rows, b.rows) and np.array_equal(a.words, b.words)


def test_filtered_model_edges():
    assign = np.array([2, 2, 0, 5, 2, 0, 9, -1], np.int32)                       # the lists of test_probe_model_edges
    ids = np.array([[1, 3, 4], [2, 2, 6], [0, 5, -1], [1 << 40, -1, 6]], np.int64)
    allow = np.array([1, 0, 2, 255, 1, 0, 1, 1], np.uint8)                       # rows 1 and 5 are not allowed
    m = probe_filtered_model(assign, 6, 2, ids, 32, allow, False)
    assert m.groups[0].rows.tolist() == [2, 0, 4, 3] and m.groups[0].words.tolist() == [4, 2, 2, 4]
    assert m.groups[0].header.tolist() == [0, 3, 4, 4, 4, 4, 4, 4, 4, 2, 0, 0, 0, 0, 0, 0]
    assert m.n_union.tolist() == [4] and m.n_allowed.tolist() == [0, 2, 2, 0]
    per = np.zeros((4, 8), bool)
    per[1, [0, 1]] = True                                                        # query 1: two rows of its cell 2
    per[2, [0, 3]] = True                                                        # query 2: row 0 is not in its cells, row 3 is
    per[0, :] = True                                                             # query 0 probes only empty cells
    m = probe_filtered_model(assign, 6, 2, ids, 32, per, True)
    assert m.groups[0].rows.tolist() == [0, 1, 3] and m.groups[0].words.tolist() == [2, 2, 4]
    assert m.groups[0].header.tolist() == [0, 1, 3, 3, 3, 3, 3, 3, 3, 2, 0, 0, 0, 0, 0, 0]
    assert m.n_allowed.tolist() == [0, 2, 1, 0]

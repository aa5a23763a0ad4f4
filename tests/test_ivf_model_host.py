"""The NumPy model of the IVF integer stages (tests/ivf_model.py) against naive loops written from include/dewi_hip.h, on tiny
inputs (no GPU).  tests/test_hip_ivf_lists.py then holds the device buffers to the model word for word."""
import numpy as np
import pytest

from ivf_model import lists_model, probe_model

INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def _naive_lists(assign, n_cells, G):
    offsets, rows = [0], []
    for cell in range(n_cells):
        for b in range(G):
            for row in range(len(assign)):
                if assign[row] == cell and row % G == b:
                    rows.append(row)
            offsets.append(len(rows))
    dropped = sum(1 for a in assign if not 0 <= a < n_cells)
    return offsets, rows, dropped


def _naive_probe(assign, n_cells, G, probe_ids, group):
    out, n_union, n_allowed = [], [], []
    for ids in probe_ids:
        mine = {int(i) for i in ids if 0 <= i < n_cells}
        n_allowed.append(sum(1 for a in assign if a in mine))
    for q0 in range(0, len(probe_ids), group):
        bits = [0] * n_cells
        for i, ids in enumerate(probe_ids[q0:q0 + group]):
            for cell in ids:
                if 0 <= cell < n_cells:
                    bits[cell] |= 1 << i
        rows, words, header = [], [], [0] * 16
        for b in range(G):
            header[b] = len(rows)
            for cell in range(n_cells):
                for row in range(len(assign)):
                    if bits[cell] and assign[row] == cell and row % G == b:
                        rows.append(row)
                        words.append(bits[cell])
        for w in range(G, 9):
            header[w] = len(rows)
        header[9] = G
        out.append((header, rows, words))
        n_union.append(len(rows))
    return out, n_union, n_allowed


def _assignments(n, n_cells, seed):
    rs = np.random.RandomState(seed)
    rand = rs.randint(0, n_cells, n).astype(np.int32)
    bad = rand.copy()
    bad[rs.choice(n, min(n, 6), replace=False)] = [-1, n_cells, INT32_MAX, INT32_MIN, -7, n_cells + 3][:min(n, 6)]
    return {"random": rand, "sorted": (np.arange(n) * n_cells // n).astype(np.int32),
            "round_robin": (np.arange(n) % n_cells).astype(np.int32), "first": np.zeros(n, np.int32),
            "last": np.full(n, n_cells - 1, np.int32), "bad": bad}


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("n,n_cells", [(1, 1), (7, 7), (64, 2), (65, 6), (200, 7), (199, 4)])
def test_lists_model_is_the_naive_sort(n, n_cells, G):
    for name, assign in _assignments(n, n_cells, seed=n + G).items():
        offsets, rows, dropped = lists_model(assign, n_cells, G)
        want = _naive_lists(assign.tolist(), n_cells, G)
        assert offsets.dtype == np.uint32 and rows.dtype == np.uint32 and offsets.shape == (n_cells * G + 1,)
        assert (offsets.tolist(), rows.tolist(), dropped) == want, name
        assert offsets[-1] == rows.size == n - dropped


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("group", [1, 3, 8, 32])
def test_probe_model_is_the_naive_expansion(G, group):
    n, n_cells = 200, 7
    rs = np.random.RandomState(10 * G + group)
    for name, assign in _assignments(n, n_cells, seed=G).items():
        for b, nprobe in ((1, 1), (group + 3, 3), (3 * group + 1, 7), (32, 5)):
            ids = rs.randint(0, n_cells, (b, nprobe)).astype(np.int64)          # repeats inside a query come by themselves
            ids[rs.rand(b, nprobe) < 0.2] = -1
            ids[rs.rand(b, nprobe) < 0.1] = n_cells
            ids[rs.rand(b, nprobe) < 0.1] = 1 << 40
            ids[b // 2] = -1                                                     # a query (for group 1: a group) with nothing valid
            if nprobe > 1:
                ids[0, 1] = ids[0, 0]
            m = probe_model(assign, n_cells, G, ids, group)
            groups, n_union, n_allowed = _naive_probe(assign.tolist(), n_cells, G, ids.tolist(), group)
            assert m.n_union.tolist() == n_union and m.n_allowed.tolist() == n_allowed, (name, b, nprobe)
            assert m.n_allowed[b // 2] == 0
            assert len(m.groups) == len(groups)
            for got, (header, rows, words) in zip(m.groups, groups):
                assert got.header.dtype == got.rows.dtype == got.words.dtype == np.uint32
                assert got.header.tolist() == header and got.rows.tolist() == rows and got.words.tolist() == words, (name, b, nprobe)


def test_probe_model_edges():
    assign = np.array([2, 2, 0, 5, 2, 0, 9, -1], np.int32)                       # cells 1, 3, 4 empty; two rows dropped (6 cells)
    m = probe_model(assign, 6, 2, np.array([[1, 3, 4], [2, 2, 6], [0, 5, -1], [1 << 40, -1, 6]], np.int64), 32)
    assert m.n_allowed.tolist() == [0, 3, 3, 0] and m.n_union.tolist() == [6]
    g = m.groups[0]
    assert g.rows.tolist() == [2, 0, 4, 5, 1, 3]                                 # bucket 0: cells 0, 2; bucket 1: cells 0, 2, 5
    assert g.words.tolist() == [4, 2, 2, 4, 2, 4]
    assert g.header.tolist() == [0, 3, 6, 6, 6, 6, 6, 6, 6, 2, 0, 0, 0, 0, 0, 0]
    empty = probe_model(assign, 6, 4, np.array([[1, 3], [4, 7]], np.int64), 8)   # only empty cells and an id out of range
    assert empty.n_union.tolist() == [0] and empty.groups[0].rows.size == 0
    assert empty.groups[0].header.tolist() == [0] * 9 + [4] + [0] * 6
    bit31 = probe_model(np.zeros(3, np.int32), 1, 1, np.zeros((32, 1), np.int64), 32)
    assert bit31.groups[0].words.tolist() == [0xFFFFFFFF] * 3

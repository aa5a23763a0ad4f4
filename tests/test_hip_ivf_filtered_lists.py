"""GPU tests of ``dewi_ivf_probe_prepare_filtered`` (csrc/ivf.hip, part (c)) at the ABI level against the NumPy model of
tests/ivf_filter_model.py, every word by exact equality.  No embeddings: an ``assign`` array, probe ids and mask bytes are all
the entry point reads.  Every case runs in a buffer with a sentinel tail the call is not told about, twice — the buffer filled
with 0xFF bytes and with random words — and the defined region (header, rows[:|U|], words[:|U|], both count arrays) must equal
the model both times.

What the shapes reach (``ivf_filter_count`` / ``ivf_filter_scan`` / ``ivf_filter_scatter``):

* blocks of the compaction: 256 positions of the UNFILTERED list U0 each.  The small cases have |U0| of a few hundred to 5000
  (2 .. 20 blocks, the last one partial); |U0| = 200000 is 782 blocks (the last holds 64 positions), 300000 is 1172.
* grid trips: count and scatter run 512 workgroups per group, 131072 positions per trip — positions 131072 .. 199999 of the
  200000-row cases are the second trip, 262144 .. 299999 of the 300000-row case the third.
* scan rounds of the block counts: 1024 blocks a round — 782 blocks are one round, 1172 blocks (300000 rows) two; the plan's own
  scan (n_cells * G words) takes 5 rounds for 1025 cells x 4.
* bucket starts: with G = 2 and 4 the unfiltered bucket boundaries (about |U0| / G, never a multiple of 256 here) lie inside a
  block; the masks "first 1000" / "last 1000" leave every bucket but the first / last empty AFTER filtering, and all-zero masks
  leave every header word to the scan kernel.
* empty blocks: "last 1000" makes the first 777 block counts zero, "first 1000" all but the first four.
"""
import ctypes

import numpy as np
import pytest

from ivf_filter_model import probe_filtered_model
from ivf_model import HEADER_WORDS, probe_model
from test_hip_ivf_lists import DIM_OF_G, SENTINEL, TAIL_WORDS, _lib, _lists, _prepare, _probes, _random

pytestmark = pytest.mark.gpu

FILLS = ("ff", "random")


def _prepare_filtered(lists_buf, n, n_cells, G, probe_ids, group, allow, per_query, fill):
    """-> (the words dewi_ivf_probe_filtered_bytes asked for, u32 words per group, out_n_union, out_n_allowed)."""
    import torch
    nat, lib = _lib()
    dim = DIM_OF_G[G]
    b, nprobe = probe_ids.shape
    need = int(lib.dewi_ivf_probe_filtered_bytes(n, dim, 0, b, group))
    stride = int(lib.dewi_ivf_probe_filtered_group_bytes(n, dim, 0, group))
    assert need > 0 and need % 4 == 0 and stride > 0 and stride % 4 == 0
    n_groups = (b + group - 1) // group
    if fill == "ff":
        body = np.full(need // 4, 0xFFFFFFFF, np.uint32)
    else:
        body = np.random.RandomState(need % 9973).randint(0, 1 << 32, need // 4, dtype=np.uint64).astype(np.uint32)
    host = np.concatenate([body, np.full(TAIL_WORDS, SENTINEL, np.uint32)])
    buf = torch.from_numpy(host.view(np.int32)).cuda()
    ids = torch.from_numpy(np.ascontiguousarray(probe_ids, dtype=np.int64)).cuda()
    mask = np.ascontiguousarray(allow).view(np.uint8) if np.asarray(allow).dtype == bool else np.ascontiguousarray(allow, np.uint8)
    assert mask.shape == ((b, n) if per_query else (n,))
    d_mask = torch.from_numpy(mask).cuda()
    n_union = (ctypes.c_int64 * n_groups)(*([-1] * n_groups))
    n_allowed = (ctypes.c_int64 * b)(*([-1] * b))
    nat.check(lib.dewi_ivf_probe_prepare_filtered(0, n, dim, nat.ptr(lists_buf), n_cells, nat.ptr(ids), b, nprobe, group,
                                                  nat.ptr(d_mask), int(per_query), nat.ptr(buf), need, n_union, n_allowed,
                                                  nat.stream_ptr()))
    torch.cuda.synchronize()
    words = buf.cpu().numpy().view(np.uint32)
    assert np.all(words[need // 4:] == SENTINEL), "a write behind the bytes dewi_ivf_probe_filtered_bytes asked for"
    return words[:need // 4], stride // 4, list(n_union), list(n_allowed)


def _check(lists_buf, assign, n_cells, G, probe_ids, group, allow, per_query=False):
    """Both fills against the model (and so against each other); -> the model."""
    n = int(assign.shape[0])
    m = probe_filtered_model(assign, n_cells, G, probe_ids, group, allow, per_query)
    defined = []
    for fill in FILLS:
        words, stride, n_union, n_allowed = _prepare_filtered(lists_buf, n, n_cells, G, probe_ids, group, allow, per_query, fill)
        assert n_union == m.n_union.tolist(), f"{fill}: out_n_union"
        assert n_allowed == m.n_allowed.tolist(), f"{fill}: out_n_allowed"
        mine = []
        for g, want in enumerate(m.groups):
            base, u = g * stride, want.rows.size
            header = words[base: base + HEADER_WORDS]
            rows = words[base + HEADER_WORDS: base + HEADER_WORDS + u]
            qwords = words[base + HEADER_WORDS + n: base + HEADER_WORDS + n + u]
            assert np.array_equal(header, want.header), f"{fill}, group {g}: header"
            assert np.array_equal(rows, want.rows), f"{fill}, group {g}: rows"
            assert np.array_equal(qwords, want.words), f"{fill}, group {g}: query words"
            assert not np.any(qwords == 0), "a listed row nobody may see"
            mine.append((header.copy(), rows.copy(), qwords.copy()))
        defined.append(mine)
    for one, two in zip(*defined):
        assert all(np.array_equal(a, b) for a, b in zip(one, two)), "the two fills differ"
    return m


# ------------------------------------------------------------------------------------------------------- 1. small cases
SMALL_N, SMALL_CELLS, UNPROBED = 5000, 37, 5


def _small(G):
    return _lists(("filtered_small", SMALL_CELLS, G, SMALL_N), lambda: _random(SMALL_N, SMALL_CELLS, seed=G), SMALL_CELLS, G)


def _small_probes(b, seed):
    ids = _probes(np.random.RandomState(seed), b, 6, SMALL_CELLS)                # invalid and repeated ids included
    ids[ids == UNPROBED] = UNPROBED + 1                                         # one cell that nobody probes
    return ids


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("b,group", [(11, 8), (11, 1), (40, 32)])
def test_shared_masks(G, b, group):
    assign, buf = _small(G)
    n = SMALL_N
    ids = _small_probes(b, seed=10 * G + group)
    rs = np.random.RandomState(b + group)
    unfiltered = probe_model(assign, SMALL_CELLS, G, ids, group)

    # all ones: what dewi_ivf_probe_prepare writes for the same probes — header, rows, words and both count arrays
    m = _check(buf, assign, SMALL_CELLS, G, ids, group, np.ones(n, np.uint8))
    words, stride, n_union, n_allowed = _prepare(buf, n, SMALL_CELLS, G, ids, group)
    assert n_union == m.n_union.tolist() == unfiltered.n_union.tolist() and n_allowed == m.n_allowed.tolist()
    for g, want in enumerate(m.groups):
        base, u = g * stride, want.rows.size
        assert np.array_equal(words[base: base + HEADER_WORDS], want.header)
        assert np.array_equal(words[base + HEADER_WORDS: base + HEADER_WORDS + u], want.rows)
        assert np.array_equal(words[base + HEADER_WORDS + n: base + HEADER_WORDS + n + u], want.words)

    # all zeros
    m = _check(buf, assign, SMALL_CELLS, G, ids, group, np.zeros(n, np.uint8))
    assert not m.n_union.any() and not m.n_allowed.any()
    assert m.groups[0].header.tolist() == [0] * 9 + [G] + [0] * 6

    # one allowed row: inside a probed cell (query 0 names cell 0), and only in the cell nobody probes
    inside = int(np.nonzero(assign == 0)[0][3])
    outside = int(np.nonzero(assign == UNPROBED)[0][0])
    for rows, total in (([inside], 1), ([outside], 0), ([inside, outside], 1)):
        mask = np.zeros(n, np.uint8)
        mask[rows] = 1
        m = _check(buf, assign, SMALL_CELLS, G, ids, group, mask)
        assert m.n_union[0] == total and m.n_allowed[0] == total
        if total:
            assert m.groups[0].rows.tolist() == [inside] and m.groups[0].words[0] & 1

    # random 1 % and 50 %; every byte value counts as "allowed" but 0
    for p in (0.01, 0.5):
        m = _check(buf, assign, SMALL_CELLS, G, ids, group, rs.rand(n) < p)
        assert 0 < m.n_union.sum() < unfiltered.n_union.sum()
    values = rs.choice(np.array([0, 1, 2, 255], np.uint8), n)
    m = _check(buf, assign, SMALL_CELLS, G, ids, group, values)
    same = probe_filtered_model(assign, SMALL_CELLS, G, ids, group, values != 0, False)
    assert m.n_allowed.tolist() == same.n_allowed.tolist() and 0 < m.n_union.sum() < unfiltered.n_union.sum()


# ------------------------------------------------------------------------------------------------------- 2. per-query masks
def _per_query_masks(rs, b, n, assign, ids):
    """Densities per query in turn: empty, one row (of a cell the query probes, where it has one), 1 %, 50 %, all."""
    masks = np.zeros((b, n), bool)
    for j in range(b):
        kind = j % 5
        if kind == 1:
            valid = ids[j][(ids[j] >= 0) & (ids[j] < SMALL_CELLS)]
            pool = np.nonzero(np.isin(assign, valid))[0] if valid.size else np.arange(n)
            masks[j, pool[rs.randint(pool.size)]] = True
        elif kind in (2, 3):
            masks[j] = rs.rand(n) < (0.01 if kind == 2 else 0.5)
        elif kind == 4:
            masks[j] = True
    return masks


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("group", [8, 1, 32])
def test_per_query_masks(G, group):
    assign, buf = _small(G)
    b, n = 11, SMALL_N
    ids = _small_probes(b, seed=100 + 10 * G + group)
    rs = np.random.RandomState(G + group)
    masks = _per_query_masks(rs, b, n, assign, ids)
    m = _check(buf, assign, SMALL_CELLS, G, ids, group, masks, per_query=True)
    unfiltered = probe_model(assign, SMALL_CELLS, G, ids, group)
    for j in range(b):                                            # |F_j| = the rows of query j's cells that ITS mask holds
        cells = ids[j][(ids[j] >= 0) & (ids[j] < SMALL_CELLS)]
        assert m.n_allowed[j] == np.count_nonzero(np.isin(assign, cells) & masks[j]), j
    assert m.n_allowed[0] == 0 and m.n_allowed[4] == unfiltered.n_allowed[4] and m.n_allowed[1] <= 1
    for g, (got, full) in enumerate(zip(m.groups, unfiltered.groups)):
        # words = bits & allow: a subset of the unfiltered list in the same order, every word a subset of the cell's bits
        where = {int(r): i for i, r in enumerate(full.rows)}
        at = np.array([where[int(r)] for r in got.rows], np.int64)
        assert np.all(np.diff(at) > 0), "the order of the unfiltered probe"
        assert np.all((got.words & ~full.words[at]) == 0) and np.all(got.words != 0)
        q0 = g * group
        allow_bits = np.zeros(got.rows.size, np.uint32)
        for i in range(min(group, b - q0)):
            allow_bits |= masks[q0 + i][got.rows].astype(np.uint32) << np.uint32(i)
        assert np.array_equal(got.words, full.words[at] & allow_bits)
    # the same masks as ONE shared mask per group of one: a prepared filter for the one-list search
    if group == 1:
        for j in (2, 3):
            one = _check(buf, assign, SMALL_CELLS, G, ids[j:j + 1], 1, masks[j])
            assert one.n_allowed[0] == m.n_allowed[j] and np.array_equal(one.groups[0].rows, m.groups[j].rows)


# ------------------------------------------------------------------------------------------------------- 3. boundaries
def _everything(n_cells, b=3):
    cells = np.arange(n_cells, dtype=np.int64)
    return np.stack([cells, np.roll(cells, 7) // 2 * 2, cells[::-1]][:b])


def test_second_grid_trip_and_many_blocks():
    n, n_cells, G = 200_000, 64, 2
    assign, buf = _lists(("random", n_cells, G, n), lambda: _random(n, n_cells, seed=G), n_cells, G)
    ids = _everything(n_cells)
    full = probe_model(assign, n_cells, G, ids, 8)
    assert full.n_union.tolist() == [n] and n > 512 * 256
    order = full.groups[0].rows.astype(np.int64)                  # the row at every unfiltered position
    rs = np.random.RandomState(5)
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[order[:1000]] = True
    last[order[-1000:]] = True
    for name, mask in (("half", rs.rand(n) < 0.5), ("first", first), ("last", last)):
        m = _check(buf, assign, n_cells, G, ids, 8, mask)
        assert m.n_union[0] == np.count_nonzero(mask), name
        assert m.n_allowed[0] == m.n_allowed[2] == m.n_union[0] and m.n_allowed[1] <= m.n_union[0]      # (query 1: even cells)
        assert name != "half" or m.n_allowed[1] < m.n_union[0]
    assert _check(buf, assign, n_cells, G, ids, 8, first).groups[0].header[1] == 1000       # bucket 1 is empty after filtering
    assert _check(buf, assign, n_cells, G, ids, 8, last).groups[0].header[1] == 0           # bucket 0 is
    per = np.stack([rs.rand(n) < 0.5, first, last])
    m = _check(buf, assign, n_cells, G, ids, 8, per, per_query=True)
    assert m.n_allowed[1] <= 1000 and m.n_allowed[2] == 1000
    _check(buf, assign, n_cells, G, ids[:1], 1, rs.rand(n) < 0.5)


def test_two_scan_rounds_of_block_counts():
    n, n_cells, G = 300_000, 64, 1                                # 1172 blocks of 256 positions: two rounds of the scan
    assign, buf = _lists(("random", n_cells, G, n), lambda: _random(n, n_cells, seed=3), n_cells, G)
    ids = _everything(n_cells, b=2)
    rs = np.random.RandomState(6)
    m = _check(buf, assign, n_cells, G, ids, 8, rs.rand(n) < 0.5)
    assert 140_000 < m.n_union[0] < 160_000
    tail = np.zeros(n, bool)
    tail[probe_model(assign, n_cells, G, ids, 8).groups[0].rows[-300:].astype(np.int64)] = True
    assert _check(buf, assign, n_cells, G, ids, 8, tail).n_union[0] == 300


def test_plan_beyond_one_scan_round():
    n, n_cells, G = 7001, 1025, 4                                 # 4100 segment sizes: the plan scans five rounds
    assign, buf = _lists(("random", n_cells, G, n), lambda: _random(n, n_cells, seed=n), n_cells, G)
    rs = np.random.RandomState(8)
    ids = _probes(rs, 11, 40, n_cells)
    m = _check(buf, assign, n_cells, G, ids, 8, rs.rand(n) < 0.5)
    assert m.n_union.min() > 0
    every = np.resize(np.arange(n_cells, dtype=np.int64), (32, -(-n_cells // 32)))
    mask = rs.rand(n) < 0.5
    m = _check(buf, assign, n_cells, G, every, 32, mask)
    assert m.n_union.tolist() == [np.count_nonzero(mask)]
    per = rs.rand(32, n) < 0.3
    _check(buf, assign, n_cells, G, every, 32, per, per_query=True)

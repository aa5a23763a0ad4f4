"""GPU tests of the two integer stages of the IVF route at the ABI level: ``dewi_ivf_lists_build`` and ``dewi_ivf_probe_prepare``
(csrc/ivf.hip) against the NumPy model of tests/ivf_model.py, every word by exact equality.  No embeddings: an ``assign``
array is all these entry points read, so the cell counts the header allows (65536 cells x 4 buckets) stay cheap.

What the shapes reach (``ivf_lists_layout`` in csrc/launch.hpp, ``block_scan_1024`` / ``ivf_copy`` in csrc/ivf.hip):

* chunk: bins <= 4096 keeps chunk 4096 (4096 bins with G = 1, 2, 4); above it chunk = bins rounded up to 64 — 4097 -> 4160,
  4100 -> 4160, 5000 -> 5056, 12000 -> 12032 (50000 rows: 5 blocks), 262144 -> 262144 (70001 rows: one block).
* scan rounds of the counts: blocks * bins words in rounds of 1024 — 5 * 12000 = 60000 words (59 rounds), 262144 (256 rounds),
  49 * 128 = 6272 for 200000 rows in 64 cells x 2.
* scan rounds of the plan: n_cells * G = 1400, 3000, 1200, 1025, 8192, 262144 -> 2, 3, 2, 2, 8, 256 rounds; the bucket heads
  b * n_cells at 1500 (round 1), 2048 / 4096 / 6144 (rounds 2, 4, 6), 65536 * b (rounds 64, 128, 192).
* copy stride: |U| = 200000 > 512 workgroups * 256 threads = 131072 list positions, so positions 131072 .. 199999 are the
  second trip of the loop.
"""
import ctypes

import numpy as np
import pytest

from ivf_model import HEADER_WORDS, lists_model, probe_model

pytestmark = pytest.mark.gpu

DIM_OF_G = {1: 64, 2: 50, 4: 129}                                            # dim matters for its G alone
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
SENTINEL = np.uint32(0xA5C3F00D)
TAIL_WORDS = 1024                                                            # 4 KiB behind what dewi_ivf_probe_bytes asks for


def _lib():
    from dewi import _native as nat
    return nat, nat.load_library()


# ------------------------------------------------------------------------------------------------------- assignments
def _random(n, n_cells, seed=0):
    return np.random.RandomState(seed).randint(0, n_cells, n).astype(np.int32)


def _sorted(n, n_cells):
    m = -(-n // n_cells)
    return (np.arange(n) // m).astype(np.int32)


def _round_robin(n, n_cells):
    return (np.arange(n) % n_cells).astype(np.int32)


def _one_cell(n, cell):
    return np.full(n, cell, np.int32)


# ------------------------------------------------------------------------------------------------------- device calls
def _build(assign, n_cells, G, fill=0):
    """dewi_ivf_lists_build -> (the buffer's u32 words on the host, the device buffer)."""
    import torch
    nat, lib = _lib()
    n, dim = int(assign.shape[0]), DIM_OF_G[G]
    assert lib.dewi_ivf_buckets(dim, 0) == G
    need = int(lib.dewi_ivf_lists_bytes(n, dim, 0, n_cells))
    assert need > 0 and need % 4 == 0
    buf = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    a = torch.from_numpy(np.ascontiguousarray(assign, dtype=np.int32)).cuda()
    nat.check(lib.dewi_ivf_lists_build(0, n, dim, n_cells, nat.ptr(a), nat.ptr(buf), need, nat.stream_ptr()))
    torch.cuda.synchronize()
    return buf.view(torch.int32).cpu().numpy().view(np.uint32), buf


def _check_lists(words, assign, n_cells, G):
    """Offsets, the listed rows and the error word against the model; -> the number of listed rows."""
    n, bins = int(assign.shape[0]), n_cells * G
    offsets, rows, dropped = lists_model(assign, n_cells, G)
    assert words[bins + 1 + n] == dropped, "the error word"
    assert np.array_equal(words[:bins + 1], offsets), "offsets"
    assert np.array_equal(words[bins + 1: bins + 1 + rows.size], rows), "rows"
    return rows.size


def _prepare(lists_buf, n, n_cells, G, probe_ids, group):
    """dewi_ivf_probe_prepare into a sentinel-filled buffer with a tail the call is not told about ->
    (words, u32 words per group, out_n_union, out_n_allowed)."""
    import torch
    nat, lib = _lib()
    dim = DIM_OF_G[G]
    b, nprobe = probe_ids.shape
    need = int(lib.dewi_ivf_probe_bytes(n, dim, 0, b, group))
    stride = int(lib.dewi_ivf_probe_group_bytes(n, dim, 0, group))
    assert need > 0 and need % 4 == 0 and stride > 0 and stride % 4 == 0
    n_groups = (b + group - 1) // group
    buf = torch.full((need // 4 + TAIL_WORDS,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")
    ids = torch.from_numpy(np.ascontiguousarray(probe_ids, dtype=np.int64)).cuda()
    n_union = (ctypes.c_int64 * n_groups)(*([-1] * n_groups))
    n_allowed = (ctypes.c_int64 * b)(*([-1] * b))
    nat.check(lib.dewi_ivf_probe_prepare(0, n, dim, nat.ptr(lists_buf), n_cells, nat.ptr(ids), b, nprobe, group, nat.ptr(buf), need,
                                         n_union, n_allowed, nat.stream_ptr()))
    torch.cuda.synchronize()
    words = buf.cpu().numpy().view(np.uint32)
    assert np.all(words[need // 4:] == SENTINEL), "a write behind the bytes dewi_ivf_probe_bytes asked for"
    return words[:need // 4], stride // 4, list(n_union), list(n_allowed)


def _check_probe(lists_buf, assign, n_cells, G, probe_ids, group):
    """Header, rows[:|U|], words[:|U|] of every group and the two returned count arrays against the model; -> the model."""
    n = int(assign.shape[0])
    words, stride, n_union, n_allowed = _prepare(lists_buf, n, n_cells, G, probe_ids, group)
    m = probe_model(assign, n_cells, G, probe_ids, group)
    assert n_union == m.n_union.tolist(), "out_n_union"
    assert n_allowed == m.n_allowed.tolist(), "out_n_allowed"
    for g, want in enumerate(m.groups):
        base, u = g * stride, want.rows.size
        assert np.array_equal(words[base: base + HEADER_WORDS], want.header), f"group {g}: header"
        assert np.array_equal(words[base + HEADER_WORDS: base + HEADER_WORDS + u], want.rows), f"group {g}: rows"
        got = words[base + HEADER_WORDS + n: base + HEADER_WORDS + n + u]
        assert np.array_equal(got, want.words), f"group {g}: query words"
    return m


def _probes(rs, b, nprobe, n_cells):
    """Random probes with everything the header says is ignored: ids outside the range, an id repeated inside a query; the
    first and the last cell are named by someone."""
    ids = rs.randint(0, n_cells, (b, nprobe)).astype(np.int64)
    ids[rs.rand(b, nprobe) < 0.08] = -1
    ids[rs.rand(b, nprobe) < 0.08] = n_cells
    ids[rs.rand(b, nprobe) < 0.08] = 1 << 40
    ids[0, 0] = 0
    ids[b - 1, nprobe - 1] = n_cells - 1
    if nprobe > 2:
        ids[0, 2] = ids[0, 1] = rs.randint(0, n_cells)
    return ids


_LISTS = {}


def _lists(key, make_assign, n_cells, G):
    """Built (and checked) once per module: (assign, device buffer)."""
    if key not in _LISTS:
        assign = make_assign()
        words, buf = _build(assign, n_cells, G)
        _check_lists(words, assign, n_cells, G)
        _LISTS[key] = (assign, buf)
    return _LISTS[key]


# ------------------------------------------------------------------------------------------------------- 1. lists build
@pytest.mark.parametrize("n_cells,G,n", [
    (4096, 1, 9001), (2048, 2, 9001), (1024, 4, 9001),         # bins = 4096: chunk stays 4096, 3 blocks
    (4097, 1, 9001),                                           # one bin more: chunk 4160
    (2050, 2, 9001),                                           # bins 4100: chunk 4160
    (5000, 1, 11000),                                          # chunk 5056, 3 blocks
    (3000, 4, 50000),                                          # bins 12000: chunk 12032, 5 blocks
    (65536, 4, 70001),                                         # bins 262144 = chunk: one block
])
def test_lists_around_the_layout_switch(n_cells, G, n):
    for assign in (_random(n, n_cells, seed=n_cells), _sorted(n, n_cells), _round_robin(n, n_cells)):
        words, _ = _build(assign, n_cells, G)
        assert _check_lists(words, assign, n_cells, G) == n


@pytest.mark.parametrize("n", [64, 65, 4095, 4096, 4097, 8192, 8193])
def test_lists_around_block_and_wave_edges(n):
    n_cells, G = 64, 2
    # round-robin over an even number of cells with G = 2: a cell owns rows of one parity, every other segment is empty
    for assign in (_random(n, n_cells, seed=n), _sorted(n, n_cells), _round_robin(n, n_cells)):
        words, _ = _build(assign, n_cells, G)
        assert _check_lists(words, assign, n_cells, G) == n
    offsets = words[:n_cells * G + 1].astype(np.int64)
    assert np.all(np.diff(offsets).reshape(n_cells, G)[np.arange(n_cells), 1 - np.arange(n_cells) % 2] == 0)


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("which", ["first", "last"])
def test_lists_everything_in_one_cell(G, which):
    n, n_cells = 200_000, 64                                   # G = 1: all 64 lanes of a wave share one bin in every round
    assign = _one_cell(n, 0 if which == "first" else n_cells - 1)
    words, _ = _build(assign, n_cells, G)
    assert _check_lists(words, assign, n_cells, G) == n


def _with_bad_entries(n, n_cells, seed):
    rs = np.random.RandomState(seed)
    assign = rs.randint(0, n_cells, n).astype(np.int32)
    bad = rs.choice(n, 97, replace=False)
    assign[bad] = np.resize(np.array([-1, n_cells, INT32_MAX, INT32_MIN], np.int32), 97)
    assign[[0, n - 1]] = [INT32_MIN, n_cells]                  # (the first and the last row among them)
    return assign, int(np.count_nonzero((assign < 0) | (assign >= n_cells)))


@pytest.mark.parametrize("n_cells,G,n", [(3000, 4, 50000), (65536, 4, 70001)])
def test_lists_drop_and_count_bad_entries(n_cells, G, n):
    assign, n_bad = _with_bad_entries(n, n_cells, seed=G)
    assert n_bad >= 97
    words, _ = _build(assign, n_cells, G)
    assert words[n_cells * G + 1 + n] == n_bad
    assert _check_lists(words, assign, n_cells, G) == n - n_bad


@pytest.mark.parametrize("n_cells,G,n", [(64, 2, 8193), (3000, 4, 50000), (64, 1, 200_000)])
def test_lists_are_deterministic(n_cells, G, n):
    assign, n_bad = _with_bad_entries(n, n_cells, seed=n)
    one, _ = _build(assign, n_cells, G, fill=0)
    two, _ = _build(assign, n_cells, G, fill=0xFF)               # whatever the buffer held before
    listed = n_cells * G + 1 + (n - n_bad)
    assert np.array_equal(one[:listed], two[:listed])
    assert one[n_cells * G + 1 + n] == two[n_cells * G + 1 + n] == n_bad
    _check_lists(two, assign, n_cells, G)


# ------------------------------------------------------------------------------------------------------- 2. probe prepare
@pytest.mark.parametrize("n_cells,G,n,b,nprobe", [
    (700, 2, 5003, 11, 40),
    (1500, 2, 9001, 11, 40),
    (300, 4, 3001, 11, 40),
    (1025, 1, 7001, 11, 40),
    (2048, 4, 12001, 11, 40),
    (65536, 4, 70001, 9, 64),
])
def test_probe_beyond_one_scan_round(n_cells, G, n, b, nprobe):
    assign, buf = _lists(("random", n_cells, G, n), lambda: _random(n, n_cells, seed=n), n_cells, G)
    rs = np.random.RandomState(n_cells)
    m = _check_probe(buf, assign, n_cells, G, _probes(rs, b, nprobe, n_cells), 8)
    assert m.n_union.min() > 0
    # every cell, shared out among one group of 32 queries: all n_cells * G segments take room, |U| = n
    every = np.resize(np.arange(n_cells, dtype=np.int64), (32, -(-n_cells // 32)))
    m = _check_probe(buf, assign, n_cells, G, every, 32)
    assert m.n_union.tolist() == [n]
    # with bad assignments in the lists: the dropped rows are in no probe
    bad_assign, n_bad = _with_bad_entries(n, n_cells, seed=G)
    words, bad_buf = _build(bad_assign, n_cells, G)
    _check_lists(words, bad_assign, n_cells, G)
    _check_probe(bad_buf, bad_assign, n_cells, G, _probes(rs, b, nprobe, n_cells), 8)


@pytest.mark.parametrize("group", [1, 5, 8, 32])
def test_probe_groups(group):
    n_cells, G, n, nprobe = 1500, 2, 9001, 12
    assign, buf = _lists(("random", n_cells, G, n), lambda: _random(n, n_cells, seed=n), n_cells, G)
    rs = np.random.RandomState(group)
    for b in (group + 3, 3 * group + 1):
        ids = _probes(rs, b, nprobe, n_cells)
        ids[1] = [-1, n_cells, 1 << 40] * (nprobe // 3)         # a query with nothing valid (group 1: a whole group)
        last = (b - 1) // group * group
        ids[last:] = -1                                         # the last group: nothing valid at all
        m = _check_probe(buf, assign, n_cells, G, ids, group)
        assert m.n_allowed[1] == 0 and m.n_union[-1] == 0 and np.all(m.n_allowed[last:] == 0)
        assert m.groups[-1].header.tolist() == [0] * 9 + [G] + [0] * 6
        assert m.n_union[0] > 0


def test_probe_every_bit_of_a_group_of_32():
    n_cells, G, n = 1500, 2, 9001
    assign, buf = _lists(("random", n_cells, G, n), lambda: _random(n, n_cells, seed=n), n_cells, G)
    shared = np.arange(100, 111, dtype=np.int64)
    ids = np.stack([np.concatenate([[40 * j + 7], shared]) for j in range(32)])      # cell 40 j + 7: query j's alone
    m = _check_probe(buf, assign, n_cells, G, ids, 32)
    seen = set(m.groups[0].words.tolist())
    assert {1 << i for i in range(32)} <= seen and 0xFFFFFFFF in seen                # each bit alone, bit 31 included


def _sparse_round_robin(n):
    return ((np.arange(n) % 8) * 8 + 3).astype(np.int32)       # cells 3, 11, .., 59 of 64 hold rows, of one parity each


@pytest.mark.parametrize("G", [1, 2, 4])
def test_probe_runs_of_empty_segments(G):
    n_cells, n = 64, 8193
    cases = {"round_robin": _round_robin(n, n_cells), "sparse": _sparse_round_robin(n)}
    for cell in (0, 20, n_cells - 1):
        cases[f"one_cell_{cell}"] = _one_cell(n, cell)
    pad = lambda cells: np.resize(np.asarray(cells, np.int64), 24)              # (a short list repeats its ids)
    for name, assign in cases.items():
        _, buf = _lists((name, n_cells, G, n), lambda: assign, n_cells, G)
        full = np.unique(assign)
        empty = np.setdiff1d(np.arange(n_cells), full)
        ids = [pad(full[::2]), pad(full[1::2] if full.size > 1 else full), pad(full[:1]), pad(full[-1:]),
               pad(np.arange(24)), pad(np.arange(40, 64)), pad(np.arange(20, 44))]
        if empty.size:
            lo, hi = empty[empty < full[0]], empty[empty > full[-1]]
            mid = empty[(empty > full[0]) & (empty < full[-1])]
            ids += [pad(part) for part in (lo, hi, mid, empty) if part.size]                         # only empty cells
            ids += [pad(np.concatenate([part[:5], full[:3], part[-5:]])) for part in (lo, hi, mid, empty) if part.size]
        ids = np.stack(ids)
        for group in (1, 8, 32):
            m = _check_probe(buf, assign, n_cells, G, ids, group)
            if empty.size:
                assert np.count_nonzero(m.n_allowed == 0) >= 2, name


@pytest.mark.parametrize("G", [1, 4])
def test_probe_copy_takes_a_second_trip(G):
    n, n_cells = 200_000, 64
    everything = np.arange(n_cells, dtype=np.int64)
    ids = np.stack([everything, np.roll(everything, 7) // 2 * 2, everything[::-1]])
    for key, make in ((("random", n_cells, G, n), lambda: _random(n, n_cells, seed=G)),
                      (("one_cell_0", n_cells, G, n), lambda: _one_cell(n, 0)),
                      (("one_cell_63", n_cells, G, n), lambda: _one_cell(n, n_cells - 1))):
        assign, buf = _lists(key, make, n_cells, G)
        m = _check_probe(buf, assign, n_cells, G, ids, 8)
        assert m.n_union.tolist() == [n] and n > 512 * 256
        m = _check_probe(buf, assign, n_cells, G, ids, 1)
        assert m.n_union[0] == m.n_union[2] == n


# ------------------------------------------------------------------------------------------------------- 3. the consumer
def test_group_of_32_feeds_the_query_filtered_search():
    """One group of 32 through dewi_knn_rerank_query_filtered == 32 groups of one through dewi_knn_rerank_filtered."""
    import torch
    from test_hip_ivf import K, _pair
    nat, lib = _lib()
    n, dim, nlist, nprobe, b = 20000, 64, 64, 4, 32
    ivf, _, Q, _ = _pair(n, dim, "cosine", seed=21, nlist=nlist, train_iters=4)
    corpus, st = ivf._corpus, ivf._ivf
    assign = ivf.cell_of_row
    probe_ids = ivf.probe(Q[:b], nprobe)
    assert len({tuple(sorted(row)) for row in probe_ids.tolist()}) > 4
    m = probe_model(assign, nlist, 1, probe_ids, 32)
    assert m.n_allowed.min() >= 2 * K, "every probe must reach the cut"
    ids_dev = torch.from_numpy(probe_ids).cuda()
    q_dev = torch.from_numpy(np.ascontiguousarray(Q[:b])).cuda()
    eta, pref, space = 0.4, 0.1, nat.SPACE_CODES["cosine"]

    def prepare(ids, group):
        nq = int(ids.shape[0])
        need = int(lib.dewi_ivf_probe_bytes(n, dim, 0, nq, group))
        buf = torch.empty(need, dtype=torch.uint8, device="cuda")
        n_union = (ctypes.c_int64 * ((nq + group - 1) // group))()
        n_allowed = (ctypes.c_int64 * nq)()
        nat.check(lib.dewi_ivf_probe_prepare(0, n, dim, nat.ptr(st.lists), nlist, nat.ptr(ids), nq, nprobe, group, nat.ptr(buf), need,
                                             n_union, n_allowed, nat.stream_ptr()))
        return buf, list(n_union), list(n_allowed)

    def workspace(n_rows_scanned, nq):
        need = int(lib.dewi_knn_filtered_workspace_bytes(n_rows_scanned, dim, nq, 2 * K))
        assert need > 0
        return torch.empty(need, dtype=torch.uint8, device="cuda")

    buf, n_union, n_allowed = prepare(ids_dev, 32)
    assert n_union == m.n_union.tolist() and n_allowed == m.n_allowed.tolist()
    got_ids = torch.full((b, K), -7, dtype=torch.int64, device="cuda")
    got_sc = torch.zeros((b, K), dtype=torch.float32, device="cuda")
    ws = workspace(n_union[0], b)
    nat.check(lib.dewi_knn_rerank_query_filtered(
        nat.ptr(corpus.emb), 0, n, dim, nat.ptr(buf), n_union[0], (ctypes.c_int64 * b)(*n_allowed), nat.ptr(q_dev), b,
        nat.ptr(corpus.dewi32), nat.ptr(corpus.ent32), K, 0, nat.SIM_CODES["ip"], eta, pref, space, nat.ptr(got_ids),
        nat.ptr(got_sc), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
    torch.cuda.synchronize()

    want_ids = torch.full((b, K), -9, dtype=torch.int64, device="cuda")
    want_sc = torch.zeros((b, K), dtype=torch.float32, device="cuda")
    stride = int(lib.dewi_ivf_probe_group_bytes(n, dim, 0, 1))
    buf1, u1, a1 = prepare(ids_dev, 1)
    assert u1 == a1 == n_allowed
    for j in range(b):
        ws1 = workspace(u1[j], 1)
        nat.check(lib.dewi_knn_rerank_filtered(
            nat.ptr(corpus.emb), 0, n, dim, nat.ptr(buf1[j * stride:]), u1[j], nat.ptr(q_dev[j:j + 1]), 1, nat.ptr(corpus.dewi32),
            nat.ptr(corpus.ent32), K, 0, nat.SIM_CODES["ip"], eta, pref, space, nat.ptr(want_ids[j:j + 1]),
            nat.ptr(want_sc[j:j + 1]), nat.ptr(ws1), ws1.numel(), nat.stream_ptr()))
    torch.cuda.synchronize()
    got_ids, want_ids = got_ids.cpu().numpy(), want_ids.cpu().numpy()
    assert np.array_equal(got_ids, want_ids)
    assert np.array_equal(got_sc.cpu().numpy().view(np.uint32), want_sc.cpu().numpy().view(np.uint32))
    for j in range(b):                                                           # ... and they are rows of the query's own cells
        assert np.all(np.isin(assign[got_ids[j]], probe_ids[j])), j

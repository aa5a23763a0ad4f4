"""The NumPy model of the collapsed re-rank (tests/collapse_model.py) on hand-worked cases and, on random records, the
properties the header's contract implies.  No GPU, no library."""
import numpy as np
import pytest

import collapse_model as cm
import rerank_model as rm

NAN, INF = float("nan"), float("inf")


def records(rows):
    return np.array(rows, dtype=rm.RECORD)


def test_hand_worked_two_per_group():
    """eta = 0: adj == sim.  Labels by id: 0,1,2 -> group 7; 3,4 -> group 9; 5 ungrouped."""
    labels = np.array([7, 7, 7, 9, 9, -1], np.int32)
    recs = records([(0.9, 0, 0, 0), (0.8, 0, 0, 3), (0.7, 0, 0, 1), (0.6, 0, 0, 2), (0.5, 0, 0, 5), (0.4, 0, 0, 4),
                    (-INF, 0, 0, -1)])
    ids, sc, hits, kk = cm.collapse_one(recs, labels, 6, 5, 2, 0.0, 0.0)
    assert ids.tolist() == [0, 3, 1, 5, 4] and kk == 5                  # id 2 is the third of group 7: folded
    assert sc.tolist() == [np.float32(x) for x in (0.9, 0.8, 0.7, 0.5, 0.4)]
    assert hits.tolist() == [3, 2, 3, 1, 2]
    ids, sc, hits, kk = cm.collapse_one(recs, labels, 6, 5, 1, 0.0, 0.0)
    assert ids.tolist() == [0, 3, 5] and kk == 3 and hits.tolist() == [3, 2, 1]
    ids, _, _, kk = cm.collapse_one(recs, labels, 6, 2, 1, 0.0, 0.0)
    assert ids.tolist() == [0, 3] and kk == 2


def test_hand_worked_blend_reorders_the_walk():
    """eta = 0.5: the second record's dewi lifts it over the first; the group's best FOR THE BLEND is the one kept."""
    labels = np.array([4, 4, 5], np.int32)
    recs = records([(0.75, 0.0, 0, 0), (0.5, 1.0, 0, 1), (0.25, 0.5, 0, 2)])
    ids, sc, hits, kk = cm.collapse_one(recs, labels, 3, 3, 1, 0.5, 0.0)
    assert ids.tolist() == [1, 2] and sc.tolist() == [0.75, 0.375] and hits.tolist() == [2, 1] and kk == 2


def test_hand_worked_padding_offset_and_extreme_labels():
    """id_offset 100, 4 rows: ids 99, 104, 2^31 - 1 and -1 are padding, whatever their sims; labels INT32_MIN / INT32_MAX."""
    labels = np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 0], np.int32)
    recs = records([(0.99, 0, 0, 99), (0.9, 0, 0, 101), (0.8, 0, 0, 104), (0.7, 0, 0, 102), (0.6, 0, 0, 2 ** 31 - 1),
                    (0.5, 0, 0, 100), (0.4, 0, 0, 103), (-INF, 0, 0, -1)])
    ids, sc, hits, kk = cm.collapse_one(recs, labels, 4, 8, 1, 0.0, 0.0, id_offset=100)
    assert ids.tolist() == [101, 100, 103] and hits.tolist() == [2, 1, 1] and kk == 3
    assert cm.valid_records(recs, 4, 100).tolist() == [1, 3, 5, 6]


def test_hand_worked_nan_and_signed_zero():
    """A NaN adj is the largest value: it is its group's first, it takes the group's place, and it is emitted last."""
    labels = np.array([1, 1, 2, 3], np.int32)
    recs = records([(NAN, 0, 0, 0), (0.5, 0, 0, 1), (-0.0, 0, 0, 2), (0.0, 0, 0, 3)])
    ids, sc, hits, kk = cm.collapse_one(recs, labels, 4, 4, 1, 0.0, 0.0)
    assert ids.tolist() == [2, 3, 0] and kk == 3                        # id 1 folded behind the NaN member of its group
    assert np.isnan(sc[2]) and sc[:2].view(np.uint32).tolist() == [0, 0]        # -0 written as +0
    ids, _, _, kk = cm.collapse_one(recs, labels, 4, 1, 1, 0.0, 0.0)
    assert ids.tolist() == [0] and kk == 1                              # NaN first in the selection: it takes the one place


def test_batch_form_prefills_and_counts():
    labels = np.zeros(5, np.int32)
    recs = records([[(0.5, 0, 0, 0), (0.4, 0, 0, 1), (0.3, 0, 0, 2)], [(-INF, 0, 0, -1)] * 3])
    ids, sc, hits, counts = cm.collapse_rerank(recs, labels, 5, 2, 1, 0.0, 0.0)
    assert ids.tolist() == [[0, -1], [-1, -1]] and counts.tolist() == [1, 0] and hits.tolist() == [[3, 0], [0, 0]]
    assert np.isnan(sc[0, 1]) and np.isnan(sc[1]).all()
    mine = np.full((2, 2), -7, np.int64)
    cm.collapse_rerank(recs, labels, 5, 2, 1, 0.0, 0.0, out_ids=mine)
    assert mine.tolist() == [[0, -7], [-7, -7]]


def random_records(rs, c, n_rows, id_offset, sort=True):
    recs = np.zeros(c, rm.RECORD)
    recs["sim"] = rs.choice(np.array([0.75, 0.5, 0.5, 0.25, 0.0, -0.0, -0.5, 0.625, NAN, INF, -INF], np.float32), c)
    recs["dewi"] = rs.choice(np.array([0.125, 0.25, 0.5, 0.875, -0.0, NAN], np.float32), c, p=[.19, .19, .19, .19, .19, .05])
    recs["ent"] = rs.rand(c).astype(np.float32)
    recs["id"] = rs.permutation(n_rows)[:c] + id_offset
    n_valid = rs.randint(1, c + 1)
    recs[n_valid:] = (-np.inf, 0.0, 0.0, -1)
    if sort:
        recs[:n_valid] = recs[:n_valid][rm.record_order(recs[:n_valid])]
    return recs


LABELLINGS = ["distinct", "equal", "negative", "few_large", "extremes"]


def make_labels(rs, kind, n_rows):
    if kind == "distinct":
        return rs.permutation(n_rows).astype(np.int32)
    if kind == "equal":
        return np.full(n_rows, 5, np.int32)
    if kind == "negative":
        return -1 - rs.randint(0, 3, n_rows).astype(np.int32)
    if kind == "few_large":
        return np.where(rs.rand(n_rows) < 0.6, rs.randint(0, 4, n_rows), 100 + np.arange(n_rows)).astype(np.int32)
    return rs.choice(np.array([-2 ** 31, -1, 0, 2 ** 31 - 1], np.int64), n_rows).astype(np.int32)


@pytest.mark.parametrize("kind", LABELLINGS)
def test_properties_on_random_records(kind):
    rs = np.random.RandomState(LABELLINGS.index(kind))
    n_rows = 300
    for trial in range(40):
        c = int(rs.choice([1, 7, 64, 200]))
        k = int(rs.choice([1, 10, c]))
        k = min(k, c)
        per_group = int(rs.choice([1, 2, 3, c]))
        eta, pref = [(0.0, 0.0), (0.3, 0.0), (0.3, 0.2)][trial % 3]
        off = [0, 1000][trial % 2]
        recs = random_records(rs, c, n_rows, off)
        labels = make_labels(rs, kind, n_rows)
        ids, sc, hits, kk = cm.collapse_one(recs, labels, n_rows, k, per_group, eta, pref, off)
        valid = recs[cm.valid_records(recs, n_rows, off)]
        n_sel = valid.shape[0]
        lab_of = {int(i): int(labels[int(i) - off]) for i in valid["id"]}
        adj = rm.blend(valid["sim"], valid["dewi"], valid["ent"], eta, pref)
        s_order = np.lexsort((np.arange(n_sel), -rm.ord32(adj).astype(np.int64)))
        s_ids = valid["id"][s_order].tolist()
        out_labels = [lab_of[i] for i in ids.tolist()]
        # every returned label at most per_group times, negative labels excepted
        for g in set(out_labels):
            if g >= 0:
                assert out_labels.count(g) <= per_group
        # the output is the S-prefix of the kept set: walking S, a record is in the output iff it fits, until kk are taken
        want, seen = [], {}
        for i in s_ids:
            g = lab_of[i]
            if g < 0 or seen.get(g, 0) < per_group:
                want.append(i)
            seen[g] = seen.get(g, 0) + 1
        want = want[:k]
        assert sorted(ids.tolist()) == sorted(want) and kk == len(want)
        nan_of = {int(i): bool(np.isnan(a)) for i, a in zip(valid["id"], adj)}
        assert ids.tolist() == [i for i in want if not nan_of[i]] + [i for i in want if nan_of[i]]
        # hits: the group's size in the pool; summed over distinct returned groups they cannot exceed the pool
        assert sum(h for g, h in {(g if g >= 0 else ("u", i)): h for g, h, i in zip(out_labels, hits.tolist(), ids.tolist())}.items()) <= n_sel
        for g, h in zip(out_labels, hits.tolist()):
            assert h == (1 if g < 0 else sum(1 for x in lab_of.values() if x == g))
        # identity 1 against the merge model
        if per_group >= n_sel or kind in ("distinct", "negative"):
            m = rm.rerank_one(recs[recs["id"] >= 0], c, k, eta, pref)
            assert m[0].tolist() == ids.tolist()
            assert np.array_equal(np.isnan(m[1]), np.isnan(sc)) and np.array_equal(m[1][~np.isnan(sc)].view(np.uint32), sc[~np.isnan(sc)].view(np.uint32))
        # identity 2
        if kind == "equal" and per_group == 1:
            assert kk == 1 and ids[0] == s_ids[0]


def test_a_group_of_nan_records_is_led_by_its_first_and_emitted_last():
    labels = np.array([3, 3, 3, 8, 8, -1], np.int32)
    recs = records([(NAN, 0.5, 0, 2), (NAN, 0.5, 0, 0), (NAN, 0.5, 0, 1), (0.5, 0.5, 0, 3), (0.25, 0.5, 0, 4), (0.125, NAN, 0, 5)])
    ids, sc, hits, kk = cm.collapse_one(recs, labels, 6, 6, 1, 0.3, 0.0)
    assert ids.tolist() == [3, 2, 5] and kk == 3 and hits.tolist() == [2, 3, 1]      # candidate rank decides among the NaN records
    assert not np.isnan(sc[0]) and np.isnan(sc[1:]).all()
    ids, _, _, kk = cm.collapse_one(recs, labels, 6, 2, 2, 0.3, 0.0)
    assert ids.tolist() == [2, 0] and kk == 2                                          # the NaN ones take the first places

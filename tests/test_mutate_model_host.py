"""The removal / upsert model of tests/mutate_model.py against hand-written examples (no GPU, no package code)."""
import numpy as np

import mutate_model as mm


def test_the_example_of_the_rule():
    # n = 6, D = {1, 4}: n' = 4, hole 1, the tail [4, 6) keeps row 5 -> 5 moves to 1
    assert mm.remove_pairs(6, [1, 4]) == ([5], [1], 4)
    assert mm.remove_order(6, [4, 1]).tolist() == [0, 5, 2, 3]


def test_deletions_only_in_the_tail_give_no_moves():
    assert mm.remove_pairs(10, [7, 8, 9]) == ([], [], 7)
    assert mm.remove_order(10, [9, 7, 8]).tolist() == list(range(7))
    assert mm.remove_pairs(10, [9]) == ([], [], 9)


def test_more_than_half_deleted_has_fewer_holes_than_deletions():
    # n = 8, D = {0, 1, 2, 5, 6}: n' = 3; holes 0, 1, 2; the tail [3, 8) keeps 3, 4, 7
    movers, holes, n_keep = mm.remove_pairs(8, [0, 1, 2, 5, 6])
    assert (movers, holes, n_keep) == ([3, 4, 7], [0, 1, 2], 3)
    assert mm.remove_order(8, [0, 1, 2, 5, 6]).tolist() == [3, 4, 7]
    # D = {2, 4, 5, 6, 7} of 8: one hole, four deletions in the tail
    movers, holes, n_keep = mm.remove_pairs(8, [2, 4, 5, 6, 7])
    assert (movers, holes, n_keep) == ([3], [2], 3) and len(holes) < 5


def test_first_and_last_rows():
    assert mm.remove_order(5, [0]).tolist() == [4, 1, 2, 3]
    assert mm.remove_order(5, [4]).tolist() == [0, 1, 2, 3]
    assert mm.remove_order(5, [0, 1, 2, 3]).tolist() == [4]
    assert mm.remove_order(5, []).tolist() == [0, 1, 2, 3, 4]


def test_movers_and_holes_never_overlap_and_survivors_are_kept_once():
    rs = np.random.RandomState(0)
    for _ in range(200):
        n = int(rs.randint(1, 60))
        m = int(rs.randint(0, n))
        dele = rs.choice(n, m, replace=False)
        movers, holes, n_keep = mm.remove_pairs(n, dele)
        assert all(s >= n_keep for s in movers) and all(h < n_keep for h in holes)
        assert movers == sorted(movers) and holes == sorted(holes)
        order = mm.remove_order(n, dele)
        assert sorted(order.tolist()) == sorted(set(range(n)) - set(dele.tolist()))


def test_ids_follow_the_rows():
    assert mm.remove_ids(list("abcdef"), ["e", "b"]) == ["a", "f", "c", "d"]


def test_upsert_keeps_known_rows_and_appends_new_ids_in_call_order():
    rows, ids = mm.upsert_rows(["a", "b", "c"], ["x", "b", "y", "a"])
    assert rows == [3, 1, 4, 0] and ids == ["a", "b", "c", "x", "y"]
    rows, ids = mm.upsert_rows([], ["p", "q"])
    assert rows == [0, 1] and ids == ["p", "q"]

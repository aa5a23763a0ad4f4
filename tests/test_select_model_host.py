"""tests/select_model.py on its own (no GPU): the consequences the contract of ``dewi_select_run`` states, on hand-made data."""
import numpy as np

import select_model as sm

INF = float("inf")


def unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def circle(angles_deg):
    a = np.deg2rad(np.asarray(angles_deg, np.float64))
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def test_lambda_one_is_a_stable_top_b():
    rs = np.random.RandomState(0)
    E = unit(rs.randn(40, 8))
    rel = rs.choice(np.array([0.5, 0.25, 0.75, 0.0, -0.0, -1.0, INF, -INF], np.float32), 40)
    rows, gains, st, _ = sm.select(E, rel, 12, 1.0)
    want = np.argsort(-sm.ord_f32(rel).astype(np.int64), kind="stable")[:12]
    assert rows.tolist() == want.tolist()
    assert np.array_equal(gains, rel[want] + np.float32(0))              # m = 1 * rel (the picked rows' pens do not count at lambda 1)
    assert st.n_picked == 12 and st.struck.sum() == 12


def test_lambda_zero_after_a_seed_is_farthest_first():
    # points on a circle: from 0 degrees the farthest is 180, then 90 before 270 (a tie: the lower row), then the 45s
    h = np.float32(np.sqrt(0.5))
    E = np.array([[1, 0], [np.cos(np.deg2rad(10)), np.sin(np.deg2rad(10))], [0, 1], [-1, 0], [0, -1], [-h, h], [h, h], [-h, -h], [h, -h]],
                 np.float32)                                              # (exact coordinates: the ties are ties in fp32 too)
    rel = np.ones(len(E), np.float32)
    rows, gains, st, _ = sm.select(E, rel, 4, 0.0, seeds=[0])
    assert rows.tolist() == [3, 2, 4, 5]
    assert np.allclose(gains, [1.0, 0.0, 0.0, -np.sqrt(0.5)], atol=1e-6)  # m = -pen = -(cosine to the nearest chosen point)
    assert st.owner[1] == 0 and st.owner[6] in (0, 2)


def test_max_sim_strikes_out_and_stays():
    E = circle([0, 5, 20, 90, 95, 180])
    rel = np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.5], np.float32)
    rows, _, st, _ = sm.select(E, rel, 6, 1.0, max_sim=float(np.cos(np.deg2rad(10))))
    assert rows.tolist() == [0, 2, 3, 5]                                 # 1 is within 10 degrees of 0, 4 of 3
    assert st.struck.all() and st.owner[1] == 0 and st.owner[4] == 3
    frozen = st.pen[1]
    assert np.isclose(frozen, np.cos(np.deg2rad(5)))                     # frozen when it was struck out: later picks do not touch it
    rows, _, st, _ = sm.select(E, rel, 6, 1.0, max_sim=-1.0)
    assert rows.tolist() == [0]                                          # every cosine is >= -1: one pick strikes everything out
    rows, _, st, _ = sm.select(E, rel, 6, 1.0, max_sim=INF)
    assert rows.tolist() == [0, 1, 2, 3, 4, 5]


def test_seeds_penalise_but_are_not_output():
    E = circle([0, 2, 90, 180])
    rel = np.array([0.5, 1.0, 0.4, 0.3], np.float32)
    rows, gains, st, _ = sm.select(E, rel, 4, 0.5, seeds=[1, 99, -1])
    assert rows.tolist() == [3, 2, 0] and st.n_picked == 3 and st.struck[1]   # (the point opposite the seed gains from a negative pen)
    assert np.isclose(gains[0], 0.5 * 0.3 - 0.5 * np.cos(np.deg2rad(178)), atol=1e-6)
    masked = np.array([1, 0, 1, 1], np.uint8)                            # a seed the mask excludes still penalises
    rows2, _, st2, _ = sm.select(E, rel, 4, 0.5, mask=masked, seeds=[1])
    assert rows2.tolist() == [3, 2, 0] and np.array_equal(st2.pen[[0, 2, 3]], st.pen[[0, 2, 3]])


def test_resume_equals_one_run():
    rs = np.random.RandomState(1)
    E = unit(rs.randn(60, 6))
    rel = rs.rand(60).astype(np.float32)
    col = sm.gram_column(E)
    whole = sm.SelectState(60)
    r, g, _ = sm.run(whole, col, rel, 25, 0.4, 0.7)
    parts = sm.SelectState(60)
    r1, g1, _ = sm.run(parts, col, rel, 9, 0.4, 0.7)
    r2, g2, _ = sm.run(parts, col, rel, 16, 0.4, 0.7)
    assert np.array_equal(np.concatenate([r1, r2]), r) and np.array_equal(np.concatenate([g1, g2]).view(np.uint32), g.view(np.uint32))
    assert np.array_equal(parts.pen.view(np.uint32), whole.pen.view(np.uint32)) and np.array_equal(parts.owner, whole.owner)
    assert parts.n_picked == whole.n_picked == len(r)


def test_nan_relevance_and_a_nan_row():
    E = circle([0, 90, 180, 270, 45])
    E[3] = np.nan
    rel = np.array([0.9, np.nan, 0.5, 0.8, 0.1], np.float32)
    rows, gains, st, _ = sm.select(E, rel, 5, 0.5)
    assert 1 not in rows.tolist() and sorted(rows.tolist()) == [0, 2, 3, 4]   # a NaN rel is never picked ...
    assert st.owner[1] >= 0 and not np.isnan(st.pen[1])                       # ... but is penalised and owned like any row
    assert np.isnan(st.pen[3]) and st.owner[3] == -1                          # the NaN row is never penalised ...
    assert not (st.owner == 3).any()                                          # ... and penalises nobody
    at = rows.tolist().index(3)
    assert gains[at] == np.float32(0.5) * np.float32(0.8)                     # its m never carries a penalty


def test_budget_above_n_and_empty_cases():
    E = circle([0, 120, 240])
    rel = np.array([0.3, 0.2, 0.1], np.float32)
    rows, _, st, _ = sm.select(E, rel, 10, 0.5)
    assert rows.tolist() == [0, 1, 2] and st.n_picked == 3
    rows, _, st, _ = sm.select(E, rel, 10, 0.5, mask=np.zeros(3, np.uint8))
    assert rows.size == 0 and st.n_picked == 0
    rows, _, _, _ = sm.select(E, rel, 0, 0.5)
    assert rows.size == 0
    rows, _, _, _ = sm.select(E, rel, 2, 0.5, id_offset=100)
    assert rows.tolist() == [100, 101]


def test_ord_round_trip_and_zero_signs():
    v = np.array([0.0, -0.0, 1.5, -1.5, INF, -INF, np.nan], np.float32)
    k = sm.ord_f32(v)
    assert k[0] == k[1] and k[6] == 0xFFFFFFFF and k[4] > k[2] > k[0] > k[3] > k[5] >= 1
    back = sm.unord_f32(k)
    assert np.array_equal(back[:6], v[:6] + np.float32(0)) and not np.signbit(back[1]) and np.isnan(back[6])


def test_float64_model_reports_the_first_undecided_pick():
    E = circle([0, 90, 180, 270])
    rel = np.array([0.5, 0.5 + 1e-6, 0.25, 0.1], np.float32).astype(np.float32)
    *_, und = sm.select(E, rel, 3, 1.0, dtype=np.float64)
    assert und == 0                                                           # 0.5 against 0.500001: inside the 2e-6 margin
    *_, und = sm.select(E, np.array([0.9, 0.5, 0.25, 0.1], np.float32), 3, 1.0, dtype=np.float64)
    assert und is None

"""The NumPy model of the int8 route (tests/int8_model.py) on its own, no GPU: the properties of the quantisation, the error
bound of a score, and the recall condition the route is offered under."""
import numpy as np
import pytest

import dewi_oracle as orc
import int8_model as im
import rerank_model as rm
from corpora import embedding_like

EPS = 2.0 ** -24


def _unit_rows(n, dim, seed):
    x = np.random.RandomState(seed).randn(n, dim)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("dim", [16, 48, 768])
def test_codes_reproduce_the_row_to_half_a_step(dim):
    x = _unit_rows(200, dim, 1) * np.float32(3.7)
    codes, scale = im.quantize(x)
    assert codes.dtype == np.int8 and scale.dtype == np.float32 and codes.shape == x.shape and scale.shape == (200,)
    assert codes.min() >= -127 and codes.max() <= 127
    # t = fl(x / scale) is off by at most |t| 2^-24 <= 127 * 2^-24, rint by at most 1/2
    err = np.abs(x.astype(np.float64) - scale.astype(np.float64)[:, None] * codes)
    assert (err <= scale.astype(np.float64)[:, None] * (0.5 + 127 * EPS)).all()
    # the largest element of a row takes the code +-127
    assert (np.abs(codes).max(axis=1) == 127).all()


def test_special_rows():
    x = _unit_rows(6, 32, 2)
    x[0, 5] = np.nan
    x[1, 7] = np.inf
    x[2, 9] = -np.inf
    x[3] = 0
    x[4] = np.float32(0.25) * np.where(np.arange(32) % 2 == 0, 1, -1)       # flat +-max
    codes, scale = im.quantize(x)
    assert np.isnan(scale[:3]).all() and (codes[:3] == 0).all()
    assert scale[3] == 0 and (codes[3] == 0).all()
    assert (np.abs(codes[4]) == 127).all() and (np.sign(codes[4]) == np.sign(x[4])).all()
    assert -128 not in codes
    # one element exactly on a .5 code boundary rounds to the even code: scale = 1 with a = 127
    y = np.zeros((1, 16), np.float32)
    y[0, 0], y[0, 1], y[0, 2], y[0, 3] = 127.0, 2.5, 3.5, -0.5
    c, s = im.quantize(y)
    assert s[0] == 1 and c[0, :4].tolist() == [127, 2, 4, 0]


def test_queries_are_normalised_before_they_are_quantised():
    q = np.random.RandomState(3).randn(4, 48).astype(np.float32) * 5
    q[2] = 0
    q[3, 4] = np.nan
    codes, scales, qn = im.prepare_query(q)
    assert np.allclose(np.linalg.norm(qn[:2].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (qn[2] == 0).all() and scales[2] == 0 and (codes[2] == 0).all()
    assert np.isnan(scales[3]) and (codes[3] == 0).all()
    want, ws = im.quantize(qn[:2])
    assert np.array_equal(codes[:2], want) and np.array_equal(scales[:2], ws)


@pytest.mark.parametrize("dim", [16, 256, 1040])
def test_score_error_bound(dim):
    """e = s_e (c_e + d_e), |d| <= 1/2: <e, q> - s_e s_q <c_e, c_q> = <e - e^, q> + <e^, q - q^>, at most
    (||q||_1 s_e + ||e^||_1 s_q) / 2 with ||e^||_1 <= ||e||_1 + dim s_e / 2 — plus fp32 rounding."""
    e = _unit_rows(300, dim, 4)
    q = _unit_rows(5, dim, 5)
    ec, es = im.quantize(e)
    qc, qs, qn = im.prepare_query(q)
    for j in range(5):
        got = im.scores(ec, es, qc[j], qs[j]).astype(np.float64)
        ref = e.astype(np.float64) @ qn[j].astype(np.float64)
        se, sq = es.astype(np.float64), float(qs[j])
        bound = (np.abs(e).sum(axis=1, dtype=np.float64) * sq + np.abs(qn[j]).sum(dtype=np.float64) * se) / 2 + dim * se * sq / 4
        slack = bound * 256 * EPS + 4 * EPS * np.abs(ref)
        assert (np.abs(got - ref) <= bound + slack).all()


def test_nan_rows_rank_first_and_ties_go_to_the_lower_row():
    e = _unit_rows(50, 32, 6)
    e[10:14] = e[3]                       # identical rows
    e[20, 0] = np.nan
    ec, es = im.quantize(e)
    qc, qs, _ = im.prepare_query(e[3:4])
    z = np.zeros(50, np.float32)
    recs = im.candidates(ec, es, qc, qs, z, z, 8, id_offset=100)
    assert recs["id"][0, 0] == 120 and recs["sim"][0, 0].view(np.uint32) == 0x7FFFFFFF
    assert recs["id"][0, 1:6].tolist() == [103, 110, 111, 112, 113]
    assert np.array_equal(rm.record_order(recs[0]), np.arange(8))
    short = im.candidates(ec[:3], es[:3], qc, qs, z[:3], z[:3], 5)
    assert (short["id"][0, 3:] == -1).all() and np.isneginf(short["sim"][0, 3:]).all()


@pytest.fixture(scope="module")
def embedding_corpus():
    X, Q, _, _ = embedding_like(20000, 256, 3)
    E = orc.build_matrix(X)
    codes, scales = im.quantize(E)
    return E, Q, codes, scales


@pytest.mark.parametrize("k", [10, 100])
def test_recall_condition(embedding_corpus, k):
    """The condition the route is offered under, on an embedding-like corpus with eta = 0: the cut c = 2k taken by the int8
    scores holds the whole exact top-k of every query, so that after re-scoring the answer is the exact one (as a set; a tie
    at the oracle's k-th place is compared by score)."""
    E, Q, codes, scales = embedding_corpus
    n = E.shape[0]
    z = np.zeros(n, np.float32)
    qc, qs, qn = im.prepare_query(Q)
    assert Q.shape[0] == 32
    recs = im.rescore(im.candidates(codes, scales, qc, qs, z, z, 2 * k), E, qn)
    ids, sc = im.search(recs, k, 0.0, 0.0)
    for j in range(32):
        ref_ids, ref_sc = orc.search(E, Q[j], z, z, k, 0.0, 0.0)
        if set(ids[j].tolist()) != set(ref_ids.tolist()):
            s64 = E.astype(np.float64) @ qn[j].astype(np.float64)
            kth = np.sort(s64)[::-1][k - 1]
            odd = np.array(sorted(set(ids[j].tolist()) ^ set(ref_ids.tolist())))
            assert (np.abs(s64[odd] - kth) <= 1e-6).all(), (j, odd)
        assert np.allclose(np.sort(sc[j]), np.sort(ref_sc), atol=1e-5)

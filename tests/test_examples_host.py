"""Search by examples, the host side (no GPU): the NumPy model against a float64 from-scratch computation and hand-made
values (both rules, both matches, the clamp, NaN propagation, -0), the Python argument checks, the three new symbols in
header / ``EXPORTED_SYMBOLS`` / library, and ``dewi_knn_examples_workspace_bytes`` without a device."""
import re
from pathlib import Path

import numpy as np
import pytest

import examples_model as xm
from rerank_model import ord32

REPO = Path(__file__).resolve().parent.parent
F = np.float32


def _lib():
    from dewi import _native as nat
    return nat, nat.load_library(require_gpu=False)


# ---------------------------------------------------------------------------------------------------------------- model
def test_prepare_examples():
    rs = np.random.RandomState(1)
    X = rs.randn(5, 132).astype(F) * F(3)
    X[1] = 0
    X[2, 7] = np.nan
    got = xm.prepare_examples(X)
    want = X[[0, 3, 4]].astype(np.float64)
    want /= np.sqrt((want ** 2).sum(axis=1, keepdims=True))
    assert np.max(np.abs(got[[0, 3, 4]] - want)) < 1.2e-7               # one rounding of the norm, one of the quotient
    assert np.array_equal(got[1], X[1]) and np.array_equal(got[2].view(np.uint32), X[2].view(np.uint32))   # left alone
    norm = F(np.sqrt(np.sum(X[0].astype(np.float64) ** 2)))
    assert np.array_equal(got[0], X[0] / norm)


def test_combine_hand_values():
    S = np.array([[0.5, 0.25, -0.5, 0.75], [0.125, 0.5, -0.25, 0.75]], F)             # two positives
    assert np.array_equal(xm.combine(S, 2), np.array([0.5, 0.5, -0.25, 0.75], F))
    assert np.array_equal(xm.combine(S, 2, match="all"), np.array([0.125, 0.25, -0.5, 0.75], F))
    # one positive, one negative
    p, n = F(0.5), np.array([0.3, -0.2, 0.0, -0.0, 0.9], F)
    S = np.stack([np.full(5, p, F), n])
    for w in (0.0, 0.5, 1.0, 2.0):
        m = np.where(n > 0, n, F(0))
        want = (p - (F(w) * m).astype(F)).astype(F)
        got = xm.combine(S, 1, negative_weight=w)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), w
        assert got[1] == p and got[2] == p and got[3] == p                                  # the clamp: a negative n costs nothing
    got = xm.combine(S, 1, negative_rule="best_score")
    assert np.array_equal(got, np.array([0.5, 0.5, 0.5, 0.5, -(F(0.9) * F(0.9))], F))
    assert xm.combine(np.array([[0.25], [0.25]], F), 1, negative_rule="best_score")[0] == -(F(0.25) * F(0.25))   # p == n: the else branch
    # two roundings, not a fused multiply-add
    p, n, w = F(1 / 3), F(0.7), F(0.3)
    got = xm.combine(np.array([[p], [n]], F), 1, negative_weight=0.3)[0]
    assert got == F(p - F(w * n))


def test_combine_nan_and_minus_zero():
    S = np.array([[0.5, np.nan, 0.5, 0.5], [0.25, 0.25, 0.25, 0.25], [0.1, 0.1, np.nan, 0.1]], F)
    for match in ("any", "all"):
        for rule in ("penalty", "best_score"):
            got = xm.combine(S, 2, match, rule, 0.0)
            assert np.array_equal(np.isnan(got), [False, True, True, False]), (match, rule)   # fmax would have dropped them
    assert np.isnan(xm.combine(S[:2], 2)[1])
    # -0: the combined score may be -0; the key's round trip gives +0, a NaN becomes 0x7FFFFFFF
    s = xm.combine(np.array([[-0.0, 0.5]], F), 1)
    rec = xm.records(np.array([-0.0, np.nan, 0.25], F), None, np.ones(3, F), np.ones(3, F), 4)
    assert s[0] == 0 and rec["id"].tolist() == [1, 2, 0, -1]
    assert rec["sim"].view(np.uint32).tolist() == [0x7FFFFFFF, F(0.25).view(np.uint32), 0, F(-np.inf).view(np.uint32)]
    assert ord32(np.array([-0.0], F))[0] == ord32(np.array([0.0], F))[0]


def test_records_order_exclusion_padding():
    score = np.array([0.5, 0.75, 0.75, np.nan, 0.25, 0.75], F)
    dewi, ent = np.arange(6, dtype=F), -np.arange(6, dtype=F)
    rec = xm.records(score, None, dewi, ent, 4, exclude=[2], id_offset=10)
    assert rec["id"].tolist() == [13, 11, 15, 10]                       # NaN on top, ties to the lower row, row 2 never offered
    assert rec["dewi"].tolist() == [3, 1, 5, 0] and rec["ent"].tolist() == [-3, -1, -5, 0]
    rec = xm.records(score[[1, 3, 4]], np.array([1, 3, 4]), dewi, ent, 5, exclude=[4, 99])    # a list; padding behind 2 offered rows
    assert rec["id"].tolist() == [3, 1, -1, -1, -1] and np.isneginf(rec["sim"][2:]).all() and not rec["dewi"][2:].any()


@pytest.mark.parametrize("match", ["any", "all"])
@pytest.mark.parametrize("rule", ["penalty", "best_score"])
def test_model_against_float64(match, rule):
    """fp32 similarities combined by the model against everything in float64 from the raw vectors: the difference is the
    fp32 rounding of the similarities (|error| <= dim * 2^-24 for unit vectors) carried through two more roundings."""
    rs = np.random.RandomState(7)
    n, dim, P, N = 300, 132, 3, 2
    E = rs.randn(n, dim)
    E = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(F)
    X = rs.randn(P + N, dim).astype(F)
    S32 = (xm.prepare_examples(X) @ E.T).astype(F)
    for w in (0.0, 0.5, 1.0, 2.0):
        got = xm.combine(S32, P, match, rule, w)
        want = xm.combine64(xm.similarities64(E, X), P, match, rule, w)
        tol = (1 + abs(w)) * (dim + 4) * 2.0 ** -24
        assert np.max(np.abs(got - want)) <= tol, (w, float(np.max(np.abs(got - want))))
    n64 = np.max(xm.similarities64(E, X)[P:], axis=0)
    p64 = (np.min if match == "all" else np.max)(xm.similarities64(E, X)[:P], axis=0)
    assert (n64 < 0).any() and (n64 > 0).any() and (p64 > n64).any() and (p64 <= n64).any()   # every branch occurs


def test_search_model_is_rerank_of_records():
    rs = np.random.RandomState(3)
    score = rs.rand(50).astype(F)
    dewi, ent = rs.rand(50).astype(F), rs.rand(50).astype(F)
    ids, sc = xm.search(score, None, dewi, ent, 20, 10, 0.0, 0.0)
    assert ids.tolist() == np.argsort(-score, kind="stable")[:10].tolist()    # eta = 0: the blend is 1 * sim
    assert np.array_equal(sc, score[ids])


# ---------------------------------------------------------------------------------------------------------------- python
def test_python_argument_checks():
    from dewi import _engine as eng
    from dewi import _native as nat
    assert eng.check_examples_request(1, 0, "any", "penalty", 1.0) == (1, 0)
    assert eng.check_examples_request(8, 8, "all", "best_score", 0) == (8, 8)
    for args in ((0, 1, "any", "penalty", 1.0), (1, -1, "any", "penalty", 1.0), (9, 8, "any", "penalty", 1.0),
                 (1, 0, "most", "penalty", 1.0), (1, 0, "any", "subtract", 1.0), (1, 1, "any", "penalty", float("nan")),
                 (1, 1, "any", "penalty", float("inf")), (1, 1, "any", "penalty", 1e300)):
        with pytest.raises(ValueError):
            eng.check_examples_request(*args)
    with pytest.raises(ValueError, match="16"):
        eng.check_examples_request(16, 1, "any", "penalty", 1.0)
    eng.check_examples_shape("cosine", False, 132)
    eng.check_examples_shape("cosine", False, 4096)
    for space, bf16, dim, word in (("l2", False, 768, "cosine"), ("cosine", True, 768, "fp32"), ("cosine", False, 128, "132"),
                                   ("cosine", False, 4100, "4096"), ("cosine", False, 766, "% 4")):
        with pytest.raises(ValueError, match=re.escape(word)):
            eng.check_examples_shape(space, bf16, dim)
    assert nat.EXAMPLES_MAX == 16 and nat.EXAMPLES_MATCH_CODES == {"any": 0, "all": 1}
    assert nat.EXAMPLES_RULE_CODES == {"penalty": 0, "best_score": 1} and eng.EXAMPLES_MAX_CANDIDATES == 2048


def test_example_parts_on_the_host():
    from dewi.backends import ExactIndex
    idx = ExactIndex(132)
    v = np.arange(132, dtype=np.float32)
    vec, rows, n_pos = idx._example_parts([v, v + 1], [v + 2])
    assert vec.shape == (3, 132) and n_pos == 2 and rows.tolist() == [-1, -1, -1] and vec[2, 0] == 2
    vec, rows, n_pos = idx._example_parts(v, None)                      # one bare vector
    assert vec.shape == (1, 132) and n_pos == 1
    vec, rows, n_pos = idx._example_parts(np.stack([v, v]), None)       # a [P, dim] array: P vectors
    assert vec.shape == (2, 132) and n_pos == 2
    with pytest.raises(ValueError):
        idx._example_parts([], [v])
    with pytest.raises(ValueError):
        idx._example_parts([v[:100]], None)
    with pytest.raises(ValueError, match="16"):
        idx._example_parts([v] * 9, [v] * 8)
    with pytest.raises(ValueError):
        idx.search_by_examples([v], match="most")
    with pytest.raises(ValueError):
        idx.search_by_examples([v], [v], negative_weight=float("nan"))
    with pytest.raises(NotImplementedError):
        idx.search_by_examples([v], filter=np.ones((2, 5), bool))


# ---------------------------------------------------------------------------------------------------------------- library
NEW_EXPORTS = {"dewi_knn_examples_workspace_bytes", "dewi_knn_candidates_examples", "dewi_examples_tuning_set"}


def test_symbols_declared_and_exported():
    nat, lib = _lib()
    header = (REPO / "include" / "dewi_hip.h").read_text()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(dewi_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(nat.EXPORTED_SYMBOLS)
    assert set(nat.EXPORTED_SYMBOLS) == declared
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
    assert "#define DEWI_EXAMPLES_MAX 16" in header
    integration = (REPO / "INTEGRATION.md").read_text()
    for name in NEW_EXPORTS:
        assert name in integration, name


def test_workspace_bytes_without_a_device():
    nat, lib = _lib()
    size = lib.dewi_knn_examples_workspace_bytes
    assert size(1000, 768, 4, 20) > 0
    # shapes the route does not take
    for n_scan, dim, n_ex, c in ((0, 768, 1, 10), (-5, 768, 1, 10), (1000, 128, 1, 10), (1000, 64, 1, 10), (1000, 766, 1, 10),
                                 (1000, 4100, 1, 10), (1000, 0, 1, 10), (1000, 768, 0, 10), (1000, 768, 17, 10),
                                 (1000, 768, 1, 0), (1000, 768, 1, 2049), (1 << 33, 768, 1, 10)):
        assert size(n_scan, dim, n_ex, c) == 0, (n_scan, dim, n_ex, c)
    for dim in (132, 256, 388, 768, 1000, 1536, 2052, 4096):
        assert size(1, dim, 1, 1) > 0 and size(63, dim, 16, 2048) > 0, dim
    # the two partial arrays are always there (8 bytes per scanned row), the keys on top; monotone in the rows and in the cut
    for dim in (132, 768, 4096):
        for c in (1, 64, 65, 256, 257, 2048):
            prev = 0
            for n_scan in (1, 63, 1000, 100_000, 5_000_000):
                got = size(n_scan, dim, 4, c)
                assert got >= 8 * n_scan and got >= prev, (dim, c, n_scan)
                prev = got
        for n_scan in (63, 100_000):
            sizes = [size(n_scan, dim, 4, c) for c in (1, 2, 64)]
            assert sizes == sorted(sizes)                                # one list per workgroup, c keys each
            sizes = [size(n_scan, dim, 4, c) for c in (65, 100, 256)]
            assert sizes == sorted(sizes)                                # one list per wave
            assert len({size(n_scan, dim, 4, c) for c in (257, 1000, 2048)}) == 1   # dense keys: one per scanned row
        # the number of examples and the pass split do not change the size
        assert len({size(100_000, dim, e, 20) for e in (1, 2, 5, 16)}) == 1
    assert lib.dewi_examples_tuning_set(2) == 0
    try:
        assert size(100_000, 768, 16, 20) == size(100_000, 768, 1, 20)
        assert lib.dewi_examples_tuning_set(-1) == nat.ERR_INVALID_ARG
    finally:
        assert lib.dewi_examples_tuning_set(0) == 0

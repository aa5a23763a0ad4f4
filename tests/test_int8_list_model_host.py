"""CPU: tests/int8_list_model.py against a naive per-query loop that scores one row at a time."""
import numpy as np
import pytest

import int8_list_model as lm
import int8_model as im
import rerank_model as rm


def naive(row_codes, row_scales, q_codes, q_scales, dewi32, ent32, c, masks, id_offset):
    b, n = q_codes.shape[0], row_codes.shape[0]
    out = []
    for j in range(b):
        mask = masks if masks.ndim == 1 else masks[j]
        scored = []
        for r in range(n):
            if not mask[r]:
                continue
            d = int(np.dot(row_codes[r].astype(np.int64), q_codes[j].astype(np.int64)))
            with np.errstate(invalid="ignore"):
                s = np.float32(np.float32(np.float32(d) * row_scales[r]) * q_scales[j])
            scored.append((-int(rm.ord32(np.array([s], np.float32))[0]), r, s))
        scored.sort(key=lambda t: (t[0], t[1]))
        recs = [(im.key_sim(s), dewi32[r], ent32[r], r + id_offset) for _, r, s in scored[:c]]
        recs += [(-np.inf, 0.0, 0.0, -1)] * (c - len(recs))
        out.append(recs)
    return np.array(out, dtype=lm.RECORD)


def corpus(n, dim, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, dim).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[10:16] = x[3]                 # ties
    x[20, 1] = np.nan               # a NaN row: first wherever it is allowed
    x[21] = 0
    codes, scales = im.quantize(x)
    q = rs.randn(3, dim).astype(np.float32)
    q[0] = x[3]
    qc, qs, _ = im.prepare_query(q)
    return codes, scales, qc, qs, rs.rand(n).astype(np.float32), rs.rand(n).astype(np.float32)


@pytest.mark.parametrize("c", [1, 7, 40, 300])
@pytest.mark.parametrize("kind", ["all", "one", "half", "random", "per_query", "empty_query"])
def test_model_equals_the_naive_loop(kind, c):
    n, dim = 120, 32
    codes, scales, qc, qs, dewi, ent = corpus(n, dim, 5)
    rs = np.random.RandomState(c)
    if kind == "all":
        masks = np.ones(n, bool)
    elif kind == "one":
        masks = np.arange(n) == 20
    elif kind == "half":
        masks = np.arange(n) % 2 == 1
    elif kind == "random":
        masks = rs.rand(n) < 0.3
    else:
        masks = rs.rand(3, n) < 0.4
        masks[1] = np.arange(n) >= 100
        if kind == "empty_query":
            masks[2] = False
    got = lm.candidates_filtered(codes, scales, qc, qs, dewi, ent, c, masks, 9)
    want = naive(codes, scales, qc, qs, dewi, ent, c, np.asarray(masks), 9)
    assert got.tobytes() == want.tobytes()


def test_every_row_is_the_unfiltered_model_and_non_members_never_appear():
    n, dim = 120, 32
    codes, scales, qc, qs, dewi, ent = corpus(n, dim, 6)
    full = lm.candidates_filtered(codes, scales, qc, qs, dewi, ent, 50, np.ones(n, bool), 4)
    assert full.tobytes() == im.candidates(codes, scales, qc, qs, dewi, ent, 50, 4).tobytes()
    mask = np.arange(n) % 3 != 0
    got = lm.candidates_filtered(codes, scales, qc, qs, dewi, ent, 100, mask)
    ids = got["id"]
    assert (ids[:, :80] % 3 != 0).all() and (ids[:, 80:] == -1).all() and np.isneginf(got["sim"][:, 80:]).all()
    # the identical rows 3, 10 .. 15 of the allowed ones, lower row first, behind the NaN row
    assert ids[0, 0] == 20 and ids[0, 1:5].tolist() == [10, 11, 13, 14]

"""NumPy model of the int8 route over allow-lists (include/dewi_hip.h, "INT8 copy, filtered"), built on tests/int8_model.py.

Query j's records are what ``int8_model.candidates`` returns for a corpus that holds only the rows of its list, with the ids
of the WHOLE corpus: non-members are removed before the cut, the order is (``ord(sim)`` desc, global row asc), padding
``(sim -inf, 0, 0, id -1)`` behind ``min(c, |list|)``.

Not a test module.
"""
import numpy as np

import int8_model as im

RECORD = im.RECORD


def candidates_filtered(row_codes, row_scales, q_codes, q_scales, dewi32, ent32, c, masks, id_offset=0):
    """Prepared queries (codes [B, dim], scales [B]) and ``masks`` — bool [n]: one list for every query, or [B, n]: one per
    query — -> records [B, c]."""
    masks = np.asarray(masks, dtype=bool)
    b, n = q_codes.shape[0], row_codes.shape[0]
    if masks.ndim == 1:
        masks = np.broadcast_to(masks, (b, n))
    assert masks.shape == (b, n)
    out = np.zeros((b, c), RECORD)
    out["sim"], out["id"] = -np.inf, -1
    for j in range(b):
        rows = np.flatnonzero(masks[j])
        if rows.shape[0] == 0:
            continue
        sub = im.candidates(row_codes[rows], row_scales[rows], q_codes[j:j + 1], q_scales[j:j + 1], dewi32[rows], ent32[rows], c)[0]
        m = min(c, rows.shape[0])
        out[j, :m] = sub[:m]
        out["id"][j, :m] = rows[sub["id"][:m]] + id_offset     # ascending rows: the local order is the global one
    return out

"""Data contract of the DEWI hot path: the per-document ``Payload`` record and the
scorer ``Weights``.

Mirrors reference ``src/dewi/types.py:8-51`` field for field (names, order, defaults,
JSON codecs) so that objects, ``payloads.jsonl`` files and keyword construction are
interchangeable with the reference.  Additions are the structure-of-arrays helpers the
device path needs: the index keeps payloads as fp32/f64 columns in HBM, not as objects.
"""
from __future__ import annotations

import dataclasses
import json
import bisect
from typing import Dict, Iterable, Iterator, List, Mapping, Optional, Sequence, Tuple

import numpy as np

#: The seven signals the scorer standardises, in the order the C ABI expects
#: (include/dewi_hip.h, DEWI_NUM_SIGNALS).
SIGNAL_FIELDS = ("ht_mean", "ht_q90", "hi_mean", "hi_q90", "I_hat", "redundancy", "noise")


@dataclasses.dataclass
class Payload:
    """Scores and signals attached to one indexed document (reference types.py:8-19)."""

    dewi: float = 0.0
    ht_mean: float = 0.0
    ht_q90: float = 0.0
    hi_mean: float = 0.0
    hi_q90: float = 0.0
    I_hat: float = 0.0
    redundancy: float = 0.0
    noise: float = 0.0

    # -- codecs (reference types.py:21-39) ------------------------------------------------
    def to_dict(self) -> Dict[str, float]:
        return {name: getattr(self, name) for name in PAYLOAD_FIELDS}

    @classmethod
    def from_dict(cls, data: Mapping[str, float]) -> "Payload":
        """Unknown keys are dropped, values go through ``float()``."""
        return cls(**{name: float(data[name]) for name in PAYLOAD_FIELDS if name in data})

    def to_bytes(self) -> bytes:
        return json.dumps(self.to_dict()).encode("utf-8")

    @classmethod
    def from_bytes(cls, data: bytes) -> "Payload":
        return cls.from_dict(json.loads(data.decode("utf-8")))


PAYLOAD_FIELDS = tuple(f.name for f in dataclasses.fields(Payload))


@dataclasses.dataclass
class Weights:
    """Scorer weights (reference types.py:42-51)."""

    alpha_t: float = 1.0
    alpha_i: float = 1.0
    alpha_m: float = 1.0
    alpha_r: float = 1.0
    alpha_n: float = 1.0
    delta: float = 3.0

    def as_vector(self) -> np.ndarray:
        """(alpha_t, alpha_i, alpha_m, alpha_r, alpha_n) as float64, the C-ABI order."""
        return np.array([self.alpha_t, self.alpha_i, self.alpha_m, self.alpha_r, self.alpha_n], dtype=np.float64)


def payload_columns(payloads: Sequence[Payload], fields: Iterable[str] = PAYLOAD_FIELDS) -> Dict[str, np.ndarray]:
    """Array-of-structs -> float64 columns (one pass per field)."""
    return {name: np.fromiter((getattr(p, name) for p in payloads), dtype=np.float64, count=len(payloads))
            for name in fields}


def payloads_from_columns(columns: Mapping[str, np.ndarray]) -> list:
    """float columns -> list of ``Payload`` (missing fields keep their 0.0 default)."""
    names = [n for n in PAYLOAD_FIELDS if n in columns]
    n = len(next(iter(columns.values()))) if columns else 0
    cols = [np.asarray(columns[name], dtype=np.float64).tolist() for name in names]
    return [Payload(**{name: col[i] for name, col in zip(names, cols)}) for i in range(n)]


class PayloadStore(dict):
    """``doc_id -> Payload`` as the reference's ``BaseIndex._payloads`` (backends.py:63), for corpora
    that may have been ingested as COLUMNS (``ExactIndex.add_batch_columns``).

    Documents added with a ``Payload`` object are plain dict entries (the object the caller passed is
    the object every lookup returns).  Column-ingested documents have no object until somebody asks
    for one: the first lookup builds a ``Payload`` from the columns and keeps it, so later lookups
    return the same object.  Bulk views (iteration, ``items``, ``values``, ``len`` is cheap) materialise
    whatever is still missing.
    """

    def __init__(self) -> None:
        super().__init__()
        self._starts: List[int] = []          # first global row of each column block
        self._blocks: List[Tuple[int, int, Sequence[str], Dict[str, np.ndarray]]] = []   # (row0, row1, ids, columns)
        self._made: List[Dict[int, "Payload"]] = []      # per block: rows that already have an object
        self._id_rows: Optional[Dict[str, int]] = None    # doc_id -> global row of column-ingested docs (lazy)
        self._lazy_count = 0
        self._owned = False                                # the blocks' arrays and id lists are the store's own (follow made them)

    # ---- ingest -----------------------------------------------------------------------------
    def add_columns(self, row0: int, doc_ids: Sequence[str], columns: Mapping[str, np.ndarray]) -> None:
        """``columns[name]``: a host array, or a CUDA tensor that STAYS on the device (``ExactIndex`` builds its HBM
        columns from it there); ``Payload`` objects of such a block are made from the handful of rows a search
        returns (one gather + one small copy, ``ensure_rows``) — only whole-store views (iteration, ``save``) bring a
        device block to the host."""
        cols = {name: (columns[name] if getattr(columns[name], "is_cuda", False) else np.asarray(columns[name], dtype=np.float64))
                for name in PAYLOAD_FIELDS if name in columns}
        n = len(doc_ids)
        for name, c in cols.items():
            if tuple(c.shape) != (n,):
                raise ValueError(f"payload column {name!r} has shape {tuple(c.shape)}, expected ({n},)")
        self._starts.append(int(row0))
        self._blocks.append((int(row0), int(row0) + n, doc_ids, cols))
        self._made.append({})
        self._id_rows = None
        self._lazy_count += n
        self._owned = False

    # ---- in-place mutation of the index (ExactIndex.remove / upsert) ----------------------------
    def _own_block(self, n_old: int) -> bool:
        """True when the store is ONE block over all ``n_old`` rows that ``follow`` made (its arrays and id list are the
        store's own): a mutation is then applied to it in place, O(rows touched) instead of a re-gather."""
        return self._owned and len(self._blocks) == 1 and self._blocks[0][0] == 0 and self._blocks[0][1] == int(n_old)

    def follow_remove(self, src: np.ndarray, dst: np.ndarray, n_old: int, doc_ids: Sequence[str], removed_ids: Sequence[str],
                      removed_rows: np.ndarray) -> None:
        """Follow ``ExactIndex.remove``: the documents ``removed_ids`` at rows ``removed_rows`` left, row ``src[i]`` moved to
        ``dst[i]``, ``doc_ids`` are the new ids in row order.  See ``follow``."""
        n_keep = int(n_old) - len(removed_ids)
        if not self._blocks:                               # a store of objects only: a plain dict
            for d in removed_ids:
                dict.pop(self, d, None)
            return
        if not self._own_block(n_old):
            order = np.arange(n_keep, dtype=np.int64)
            order[dst] = src
            return self.follow(order, n_old, doc_ids, removed=removed_ids)
        for d in removed_ids:
            dict.pop(self, d, None)
        _, _, ids, cols = self._blocks[0]
        made = self._made[0]
        for name, c in list(cols.items()):
            if len(src):
                if getattr(c, "is_cuda", False):
                    import torch
                    s_t, d_t = torch.from_numpy(np.ascontiguousarray(src)).to(c.device), torch.from_numpy(np.ascontiguousarray(dst)).to(c.device)
                    c.index_copy_(0, d_t, c.index_select(0, s_t))
                else:
                    c[dst] = c[src]
            cols[name] = c[:n_keep]
        for r in np.asarray(removed_rows).tolist():
            made.pop(r, None)
        for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
            p = made.pop(s, None)
            if p is not None:
                made[d] = p
            ids[d] = ids[s]
        del ids[n_keep:]
        self._blocks[0] = (0, n_keep, ids, cols)
        self._id_rows = None
        self._lazy_count = n_keep - len(made)

    def follow_put(self, rows: np.ndarray, n_old: int, doc_ids: Sequence[str], ids: Sequence[str], objects=None, columns=None) -> None:
        """Follow ``ExactIndex.upsert_batch`` / ``upsert_batch_columns``: document ``ids[i]`` was written to row ``rows[i]``
        (rows from ``n_old`` on are new), with ``objects[i]`` as its ``Payload`` or row i of ``columns`` ({field: values}, host
        or CUDA).  See ``follow``."""
        rows = np.asarray(rows, dtype=np.int64)
        n_new = len(doc_ids)
        if not self._blocks and columns is None:
            for d, p in zip(ids, objects):
                dict.__setitem__(self, d, p)
            return
        if not self._own_block(n_old):
            order = np.concatenate([np.arange(int(n_old), dtype=np.int64), np.full(n_new - int(n_old), -1, dtype=np.int64)])
            order[rows] = -1
            if objects is not None:
                return self.follow(order, n_old, doc_ids, objects=list(zip(rows.tolist(), ids, objects)))
            return self.follow(order, n_old, doc_ids, columns=(rows, ids, columns))
        _, _, own_ids, cols = self._blocks[0]
        made = self._made[0]
        grown = n_new - int(n_old)
        names = [name for name in PAYLOAD_FIELDS if name in cols or (columns is not None and name in columns)]
        for name in names:
            c = cols.get(name)
            vals = None if columns is None else columns.get(name)
            if c is None:
                c = np.zeros(int(n_old), dtype=np.float64)
            if getattr(vals, "is_cuda", False) and not getattr(c, "is_cuda", False):
                import torch
                c = torch.from_numpy(c).to(vals.device)           # a column with device values lives on the device from now on
            if getattr(c, "is_cuda", False):
                import torch
                if grown:
                    c = torch.cat([c, torch.zeros(grown, dtype=c.dtype, device=c.device)])
                at = torch.from_numpy(rows).to(c.device)
                v = (torch.zeros(len(rows), dtype=c.dtype, device=c.device) if vals is None
                     else (vals if getattr(vals, "is_cuda", False) else torch.from_numpy(np.asarray(vals, dtype=np.float64))).to(device=c.device, dtype=c.dtype))
                c.index_copy_(0, at, v)
            else:
                if grown:
                    c = np.concatenate([c, np.zeros(grown, dtype=np.float64)])
                c[rows] = 0.0 if vals is None else np.asarray(vals, dtype=np.float64)
            cols[name] = c
        if objects is not None:
            for r, d, p in zip(rows.tolist(), ids, objects):
                dict.__setitem__(self, d, p)
                made[r] = p
        else:
            for r, d in zip(rows.tolist(), ids):
                dict.pop(self, d, None)       # a replaced document's old object: the next lookup makes one from the new columns
                made.pop(r, None)
        own_ids.extend(doc_ids[int(n_old):])
        self._blocks[0] = (0, n_new, own_ids, cols)
        self._id_rows = None
        self._lazy_count = n_new - len(made)

    def follow(self,order: np.ndarray, n_old: int, doc_ids: Sequence[str], removed: Iterable[str] = (),
               objects: Sequence[Tuple[int, str, "Payload"]] = (), columns=None) -> None:
        """Follow a mutation of the index.  ``order`` int64 [n_new]: the OLD row whose document now sits at each new row, or
        -1 where the row's payload is new; ``n_old``: rows before; ``doc_ids``: the new ids in row order; ``removed``: ids
        that left; ``objects``: ``(row, doc_id, Payload)`` of new payloads given as objects; ``columns``: ``(rows, doc_ids,
        {field: values})`` of new payloads given as columns (host arrays or CUDA tensors).

        Dict entries are deleted or replaced; ``Payload`` objects already handed out for surviving documents stay the same
        objects.  Column blocks are re-gathered into the new row order — host columns with NumPy, device columns with
        ``index_select``, both as float64 (exact for fp32 columns) — into ONE block over all rows, in which rows that have an
        object are listed as made.  That is O(N) host work per call (not per row), plus one gather per column.  The block it
        leaves is the store's own, and ``follow_remove`` / ``follow_put`` apply later mutations to it in place, in O(rows
        touched) (an append copies the columns once more to make room)."""
        order = np.asarray(order, dtype=np.int64)
        n_new = int(order.shape[0])
        for d in removed:
            dict.pop(self, d, None)
        for _, d, p in objects:
            dict.__setitem__(self, d, p)
        if columns is not None:
            for d in columns[1]:
                dict.pop(self, d, None)       # a replaced document's old object: the next lookup makes one from the new columns
        if not self._blocks and columns is None:
            return
        alive = order >= 0
        inv = np.full(int(n_old), -1, dtype=np.int64)
        inv[order[alive]] = np.flatnonzero(alive)
        # per old block: the new rows it fills and the block-local rows they come from
        takes = []
        in_block = np.zeros(n_new, dtype=bool)
        for row0, row1, _, _ in self._blocks:
            dst = np.flatnonzero(alive & (order >= row0) & (order < row1))
            takes.append((dst, order[dst] - row0))
            in_block[dst] = True
        names = [name for name in PAYLOAD_FIELDS
                 if any(name in b[3] for b in self._blocks) or (columns is not None and name in columns[2])]
        new_cols: Dict[str, np.ndarray] = {}
        for name in names:
            parts = [(dst, src, b[3][name]) for (dst, src), b in zip(takes, self._blocks) if name in b[3]]
            if columns is not None and name in columns[2]:
                parts.append((np.asarray(columns[0], dtype=np.int64), None, columns[2][name]))
            dev = next((c.device for _, _, c in parts if getattr(c, "is_cuda", False)), None)
            if dev is None:
                out = np.zeros(n_new, dtype=np.float64)
                for dst, src, c in parts:
                    c = np.asarray(c, dtype=np.float64)
                    out[dst] = c if src is None else c[src]
            else:
                import torch
                out = torch.zeros(n_new, dtype=torch.float64, device=dev)
                for dst, src, c in parts:
                    c = c if getattr(c, "is_cuda", False) else torch.from_numpy(np.asarray(c, dtype=np.float64)).to(dev)
                    if src is not None:
                        c = c.index_select(0, torch.from_numpy(src).to(dev))
                    out.index_copy_(0, torch.from_numpy(np.ascontiguousarray(dst)).to(dev), c.to(torch.float64))
            new_cols[name] = out
        made: Dict[int, "Payload"] = {}
        for old_made in self._made:
            for row, p in old_made.items():
                if inv[row] >= 0:
                    made[int(inv[row])] = p
        for row in np.flatnonzero(alive & ~in_block).tolist():       # documents that came with an object
            made[row] = dict.__getitem__(self, doc_ids[row])
        for row, _, p in objects:
            made[int(row)] = p
        self._starts = [0]
        self._blocks = [(0, n_new, list(doc_ids), new_cols)]
        self._made = [made]
        self._id_rows = None
        self._lazy_count = n_new - len(made)
        self._owned = True

    # ---- row access (search results: no doc_id -> row map needed) -----------------------------
    def _block_of(self, row: int) -> int:
        j = bisect.bisect_right(self._starts, row) - 1
        if j < 0 or row >= self._blocks[j][1]:
            return -1
        return j

    def at_row(self, row: int, doc_id: str) -> "Payload":
        hit = dict.get(self, doc_id)
        if hit is not None:
            return hit
        j = self._block_of(row)
        if j < 0:
            raise KeyError(doc_id)
        return self._make(j, row, doc_id)

    def _block_on_device(self, j: int) -> bool:
        return any(getattr(c, "is_cuda", False) for c in self._blocks[j][3].values())

    def _block_to_host(self, j: int) -> None:
        row0, row1, ids, cols = self._blocks[j]
        self._blocks[j] = (row0, row1, ids, {name: (c.detach().cpu().numpy().astype(np.float64) if getattr(c, "is_cuda", False) else c)
                                             for name, c in cols.items()})

    def ensure_rows(self, rows: Sequence[int], doc_ids: Sequence[str]) -> None:
        """Make the ``Payload`` objects of ``rows`` that live in device-resident column blocks: per block ONE gather
        of the wanted rows over all its columns and one small device-to-host copy."""
        want: Dict[int, List[int]] = {}
        for row in rows:
            if dict.__contains__(self, doc_ids[row]):
                continue
            j = self._block_of(row)
            if j >= 0 and row not in self._made[j] and self._block_on_device(j):
                want.setdefault(j, []).append(row)
        if not want:
            return
        import torch
        for j, rws in want.items():
            row0, _, _, cols = self._blocks[j]
            rws = sorted(set(rws))
            names = list(cols)
            dev = next(c.device for c in cols.values() if getattr(c, "is_cuda", False))
            idx = torch.tensor([r - row0 for r in rws], dtype=torch.int64, device=dev)
            block = torch.stack([(c if getattr(c, "is_cuda", False) else torch.from_numpy(c).to(dev)).index_select(0, idx).double()
                                 for c in cols.values()]).cpu().numpy()
            for t, row in enumerate(rws):
                p = Payload(**{name: float(block[f, t]) for f, name in enumerate(names)})
                dict.__setitem__(self, doc_ids[row], p)
                self._made[j][row] = p
                self._lazy_count -= 1

    def _make(self, j: int, row: int, doc_id: str) -> "Payload":
        row0, _, _, cols = self._blocks[j]
        p = Payload(**{name: float(c[row - row0]) for name, c in cols.items()})
        dict.__setitem__(self, doc_id, p)
        self._made[j][row] = p
        self._lazy_count -= 1
        return p

    def column_blocks(self) -> Iterator[Tuple[int, int, Dict[str, np.ndarray], Dict[int, "Payload"]]]:
        """(row0, row1, columns, objects already handed out for rows of the block)."""
        for (row0, row1, _, cols), made in zip(self._blocks, self._made):
            yield row0, row1, cols, made

    # ---- mapping protocol -----------------------------------------------------------------------
    def _rows_by_id(self) -> Dict[str, int]:
        if self._id_rows is None:
            m: Dict[str, int] = {}
            for row0, _, ids, _ in self._blocks:
                m.update(zip(ids, range(row0, row0 + len(ids))))
            self._id_rows = m
        return self._id_rows

    def __missing__(self, doc_id: str) -> "Payload":
        row = self._rows_by_id().get(doc_id) if self._blocks else None
        if row is None:
            raise KeyError(doc_id)
        return self._make(self._block_of(row), row, doc_id)

    def get(self, doc_id, default=None):
        try:
            return self[doc_id]
        except KeyError:
            return default

    def __contains__(self, doc_id) -> bool:
        return dict.__contains__(self, doc_id) or (bool(self._blocks) and doc_id in self._rows_by_id())

    def __len__(self) -> int:
        return dict.__len__(self) + self._lazy_count

    def materialize_all(self) -> None:
        if self._lazy_count:
            for j in range(len(self._blocks)):
                if self._block_on_device(j):
                    self._block_to_host(j)        # a whole-store view: the block's columns come over once
            for j, (row0, _, ids, _) in enumerate(self._blocks):
                made = self._made[j]
                for i, doc_id in enumerate(ids):
                    if row0 + i not in made and not dict.__contains__(self, doc_id):
                        self._make(j, row0 + i, doc_id)
            self._lazy_count = 0

    def __iter__(self):
        self.materialize_all()
        return dict.__iter__(self)

    def keys(self):
        self.materialize_all()
        return dict.keys(self)

    def values(self):
        self.materialize_all()
        return dict.values(self)

    def items(self):
        self.materialize_all()
        return dict.items(self)

"""Index backends of the MI355X-native DEWI drop-in.

Same module name and public surface as reference ``src/dewi/backends.py`` —
``IndexBackend``, ``BaseIndex``, ``ExactIndex``, ``HNSWIndex``, ``FAISSIndex`` and the
``_HAS_HNSW`` / ``_HAS_FAISS`` flags — but ``ExactIndex`` is the brute-force index
re-designed for the GPU: the embedding matrix and the payload columns live in HBM and
``search`` is two HIP kernel launches (see ``csrc/knn_scan.hip`` and
``csrc/select_rerank.hip``).  There is no CPU search path: without the HIP extension or
without a GPU, ``build``/``search`` raise ``NativeLibraryError``.

The approximate backends (hnswlib / faiss graphs) are outside the hot path this package
rebuilds; their classes exist so that imports keep working and raise ``ImportError`` on
construction, which is what the reference does when those libraries are not installed
(backends.py:171-172, 249-250).
"""
from __future__ import annotations

import dataclasses
import enum
import json
import logging
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .attributes import AttributesMixin
from .types import PAYLOAD_FIELDS, Payload, PayloadStore, payload_columns
from .where import Where, is_where_list

logger = logging.getLogger(__name__)

# ANN libraries are not part of this build (graph indexes are out of scope).
_HAS_HNSW = False
_HAS_FAISS = False


class IndexBackend(enum.Enum):
    """Backend selector (reference backends.py:32-49).  ``AUTO`` resolves to the HIP exact index."""

    HNSW = enum.auto()
    FAISS_IVFFLAT = enum.auto()
    FAISS_HNSW = enum.auto()
    EXACT = enum.auto()

    @classmethod
    def from_str(cls, name: str) -> "IndexBackend":
        key = name.upper()
        if key == "AUTO":
            return cls.EXACT
        return cls[key]  # KeyError for unknown names, as in the reference


SearchResult = List[Tuple[str, float, Payload]]


def clusters_from_labels(labels: np.ndarray, doc_ids: Sequence[str]) -> List[List[str]]:
    """Group labels int64 [N] -> the groups as lists of doc ids: ordered by label, members by ascending row, singletons
    included.  Host logic only."""
    labels = np.asarray(labels)
    if labels.size == 0:
        return []
    order = np.argsort(labels, kind="stable")
    cuts = np.flatnonzero(np.diff(labels[order])) + 1
    return [[doc_ids[i] for i in grp.tolist()] for grp in np.split(order, cuts)]


@dataclasses.dataclass
class DuplicateGroups:
    """``ExactIndex.duplicate_groups``: per row the group's label (its smallest row), its size and its representative row —
    numpy int64 [N] — the number of groups (singletons included), and with ``doc_ids=True`` the groups as lists of doc ids
    (ordered by label, members by ascending row, singletons included), else ``None``."""

    labels: np.ndarray
    sizes: np.ndarray
    representatives: np.ndarray
    n_groups: int
    clusters: Optional[List[List[str]]] = None


class BaseIndex:
    """Backend contract (reference backends.py:54-163): add / build / search / save / load."""

    def __init__(self, dim: int, space: str = "cosine", **kwargs: Any):
        self.dim = dim
        self.space = space
        self._index = None
        self._doc_ids: List[str] = []
        self._payloads: Dict[str, Payload] = {}
        self._is_trained = False

    def add(self, doc_id: str, embedding: np.ndarray, payload: Payload) -> None:
        raise NotImplementedError

    def build(self, **kwargs: Any) -> None:
        raise NotImplementedError

    def search(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0) -> SearchResult:
        raise NotImplementedError

    # Generic persistence: metadata + payloads only (reference backends.py:104-163, key "id").
    def save(self, path: Union[str, Path]) -> None:
        root = Path(path)
        root.mkdir(parents=True, exist_ok=True)
        with open(root / "payloads.jsonl", "w") as fh:
            for doc_id in self._doc_ids:
                fh.write(json.dumps({"id": doc_id, "payload": self._payloads[doc_id].to_dict()}) + "\n")
        with open(root / "metadata.json", "w") as fh:
            json.dump({"dim": self.dim, "space": self.space, "doc_ids": self._doc_ids,
                       "is_trained": self._is_trained, "type": type(self).__name__}, fh)

    @classmethod
    def load(cls, path: Union[str, Path], **kwargs: Any) -> "BaseIndex":
        root = Path(path)
        with open(root / "metadata.json") as fh:
            meta = json.load(fh)
        target = globals().get(meta.get("type", ""), cls)
        inst = target(dim=meta["dim"], space=meta["space"], **kwargs)
        inst._doc_ids = meta["doc_ids"]
        inst._is_trained = meta["is_trained"]
        with open(root / "payloads.jsonl") as fh:
            for line in fh:
                rec = json.loads(line)
                inst._payloads[rec["id"]] = Payload.from_dict(rec["payload"])
        return inst


def filter_kwargs(filter) -> Dict[str, Any]:
    """What an unprepared ``filter=`` argument is, as ``make_filter`` keywords: a bool array is a mask, strings are doc
    ids, integers are row positions."""
    if isinstance(filter, str):
        return {"doc_ids": [filter]}
    if hasattr(filter, "dtype"):
        return {"mask": filter} if "bool" in str(filter.dtype) else {"rows": filter}
    items = list(filter)
    if items and all(isinstance(x, str) for x in items):
        return {"doc_ids": items}
    arr = np.asarray(items)
    if arr.dtype == np.bool_:
        return {"mask": arr}
    return {"rows": arr.astype(np.int64) if arr.size else np.zeros(0, np.int64)}


class HNSWIndex(BaseIndex):
    """hnswlib graph index — not part of this build (reference backends.py:166-241)."""

    def __init__(self, dim: int, space: str = "cosine", M: int = 16, ef_construction: int = 200, **kwargs: Any):
        super().__init__(dim, space, **kwargs)
        raise ImportError("HNSW not available in the MI355X build: use ExactIndex (HIP brute force)")


class FAISSIndex(BaseIndex):
    """faiss index — not part of this build (reference backends.py:244-383)."""

    def __init__(self, dim: int, space: str = "cosine", index_type: str = "IVFFlat", nlist: int = 100, **kwargs: Any):
        super().__init__(dim, space, **kwargs)
        raise ImportError("FAISS not available in the MI355X build: use ExactIndex (HIP brute force)")


class ExactIndex(AttributesMixin, BaseIndex):
    """Exact nearest-neighbour search with DEWI re-ranking, on the GPU.

    Drop-in for reference ``ExactIndex`` (backends.py:386-556): same constructor, same
    ``add``/``build``/``search`` semantics (top-``min(2k, N)`` by similarity, then the
    eta blend, then top-k), same on-disk format.  Differences, all additive:

    * ``add_batch`` / ``search_batch`` bulk entry points (the reference is one row / one
      query per call), and ``add_batch_columns`` (payloads as arrays: no Python object per row;
      ``Payload`` objects are made on demand for the rows a search returns);
    * rows are normalised by a device kernel at ``build`` (not on the host at ``add``), so
      stored rows can differ from the reference's in the last fp32 bit;
    * the payload values the re-rank reads (``dewi``, ``ht_mean``, ``hi_mean``) are
      snapshotted into HBM columns at ``build``; call ``refresh_payloads()`` after mutating
      ``Payload`` objects in place;
    * attribute columns and predicates over them (``set_attributes``, ``make_filter_where``, ``filter=`` a
      ``dewi.where.Where``): ``dewi.attributes.AttributesMixin``.
    """

    def __init__(self, dim: int, space: str = "cosine", **kwargs: Any):
        super().__init__(dim, space, **kwargs)
        self._payloads = PayloadStore()            # a dict (reference contract) that also serves column-ingested rows
        self._normalize = space == "cosine"
        self._pending: List[np.ndarray] = []      # raw fp32 rows (or [m, d] blocks) not yet on the device
        self._pending_rows = 0
        self._corpus = None                        # _engine.DeviceCorpus once built
        self._host_rows: Optional[np.ndarray] = None  # lazily materialised copy of the stored matrix
        self._loaded_rows: Optional[np.ndarray] = None  # rows read by load(): already in stored form
        self._device: Optional[str] = kwargs.get("device")
        # additive: keep a bf16 shadow copy of the fp32 matrix (+50 % HBM): search_batch then runs a matrix-core pass over the
        # copy as a pre-selection (half the bytes; 256 queries per corpus pass above 32) and re-scores the candidates from the
        # fp32 rows — same ids and scores as the one-query search (DeviceCorpus.enable_bf16_shadow)
        self._batch_shadow: bool = bool(kwargs.get("batch_shadow", False))
        # with batch_shadow: search() of ONE query goes through the shadow too (same answers; see enable_bf16_shadow)
        self._shadow_single: bool = bool(kwargs.get("shadow_single_query", False))
        # additive: keep an int8 copy of the fp32 matrix (+25 % HBM) for the APPROXIMATE route — search(approx=...) takes the
        # candidate cut by integer scores over a quarter of the bytes and re-scores it from the fp32 rows
        # (DeviceCorpus.enable_int8_shadow).  remove / upsert* mark the copy stale: the next approximate search re-quantises
        # the whole matrix (one pass over the fp32 rows), so a mutated index and a fresh one answer bit-equally.
        self._int8_shadow: bool = bool(kwargs.get("int8_shadow", False))
        if self._int8_shadow:
            from ._engine import check_int8_shape
            check_int8_shape(space, False, dim)
        # additive: keep a 1-bit copy of the fp32 matrix (the signs, +3 % HBM) for search_binary: the candidate cut by Hamming
        # distance over 1 / 32 of the bytes, re-scored from the fp32 rows (DeviceCorpus.enable_binary_shadow).  Nothing routes
        # there by itself; remove / upsert* mark the copy stale exactly as they mark the int8 copy.
        self._binary_shadow: bool = bool(kwargs.get("binary_shadow", False))
        if self._binary_shadow:
            from ._engine import check_binary_shape
            check_binary_shape(space, False, dim)
        self._id_rows: Optional[Dict[str, int]] = None  # doc_id -> row of remove / upsert: made once, then kept per call
        self._attrs_init()                          # attribute columns (dewi.attributes)

    # ---------------------------------------------------------------- ingest (A1)
    def add(self, doc_id: str, embedding: np.ndarray, payload: Payload) -> None:
        if embedding.shape != (self.dim,):
            raise ValueError(f"Expected embedding of shape {(self.dim,)}, got {embedding.shape}")
        self._doc_ids.append(doc_id)
        self._payloads[doc_id] = payload
        self._pending.append(np.array(embedding, dtype=np.float32))
        self._pending_rows += 1
        self._invalidate()

    def add_batch(self, doc_ids: Sequence[str], embeddings: np.ndarray, payloads: Sequence[Payload]) -> None:
        """Bulk ``add``: ``embeddings`` is [m, dim]; one shape check, no per-row Python work."""
        emb = np.asarray(embeddings)
        if emb.ndim != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"Expected embeddings of shape (m, {self.dim}), got {emb.shape}")
        if not (len(doc_ids) == emb.shape[0] == len(payloads)):
            raise ValueError("doc_ids, embeddings and payloads must have the same length")
        self._doc_ids.extend(doc_ids)
        self._payloads.update(zip(doc_ids, payloads))
        self._pending.append(np.array(emb, dtype=np.float32))
        self._pending_rows += emb.shape[0]
        self._invalidate()

    def add_batch_columns(self, doc_ids: Sequence[str], embeddings: np.ndarray, columns: Dict[str, np.ndarray],
                          copy: bool = False) -> None:
        """Bulk ``add`` with the payloads as structure-of-arrays: ``columns[name]`` is one
        float array per ``Payload`` field (missing fields are 0.0, as ``Payload()``'s defaults).  Nothing
        is done per row in Python: a 1 M-row ingest is a list extend plus array bookkeeping, and
        ``build`` uploads the columns as they are.  ``Payload`` objects are created lazily — for the
        rows a search returns, or on ``get_payload`` / iteration over ``_payloads`` — and the same
        object is returned from then on.  ``copy=False``: the embedding block is referenced, not
        copied, until ``build()``; do not modify it in between.

        DEVICE-RESIDENT ingest: ``embeddings`` may be a CUDA fp32 tensor [m, dim] and the columns CUDA tensors (the
        ``dewi32`` column of ``DewiScorer.score_batch_device``, signal columns ...).  Nothing is copied to the host;
        when the block is the whole corpus ``build()`` uses it IN PLACE — cosine rows are normalised inside the
        caller's tensor (``copy=True`` keeps the caller's tensor intact at the price of a device copy) — and the
        HBM payload columns are computed on the device from the given columns."""
        from . import _native as nat
        if nat.is_device_tensor(embeddings):
            return self._add_device_block(doc_ids, embeddings, columns, copy)
        emb = np.asarray(embeddings)
        if emb.ndim != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"Expected embeddings of shape (m, {self.dim}), got {emb.shape}")
        if len(doc_ids) != emb.shape[0]:
            raise ValueError("doc_ids and embeddings must have the same length")
        unknown = [name for name in columns if name not in PAYLOAD_FIELDS]
        if unknown:
            raise ValueError(f"unknown payload columns {unknown}")
        row0 = len(self._doc_ids)
        self._payloads.add_columns(row0, doc_ids, columns)         # validates the column shapes
        self._doc_ids.extend(doc_ids)
        self._pending.append(np.array(emb, dtype=np.float32) if copy else np.ascontiguousarray(emb, dtype=np.float32))
        self._pending_rows += emb.shape[0]
        self._invalidate()

    def _add_device_block(self, doc_ids: Sequence[str], embeddings, columns, copy: bool) -> None:
        import torch
        emb = embeddings
        if emb.dim() != 2 or int(emb.shape[1]) != self.dim:
            raise ValueError(f"Expected embeddings of shape (m, {self.dim}), got {tuple(emb.shape)}")
        if len(doc_ids) != int(emb.shape[0]):
            raise ValueError("doc_ids and embeddings must have the same length")
        unknown = [name for name in columns if name not in PAYLOAD_FIELDS]
        if unknown:
            raise ValueError(f"unknown payload columns {unknown}")
        if emb.dtype != torch.float32 or not emb.is_contiguous():
            emb = emb.to(dtype=torch.float32).contiguous()                 # a device copy: no longer the caller's tensor
        elif copy:
            emb = emb.clone()
        row0 = len(self._doc_ids)
        self._payloads.add_columns(row0, doc_ids, columns)
        self._doc_ids.extend(doc_ids)
        self._pending.append(emb)
        self._pending_rows += int(emb.shape[0])
        self._invalidate()

    def _invalidate(self) -> None:
        self._is_trained = False
        self._host_rows = None
        self._id_rows = None

    # ---------------------------------------------------------------- remove / upsert in place (additive)
    @property
    def capacity(self) -> int:
        """Rows the device storage holds without reallocating (0 before the first build)."""
        return 0 if self._corpus is None else self._corpus.capacity

    def reserve(self, rows: int) -> None:
        """Make room on the device for ``rows`` documents, so that upserts of new ids up to there do not reallocate
        (``DeviceCorpus.reserve``: a device-to-device copy, peak memory old plus new; the storage never shrinks)."""
        self._ensure_built()
        self._corpus.reserve(int(rows))
        self._attr_columns()                        # (the attribute columns grow with the storage)

    def _row_map(self) -> Dict[str, int]:
        """doc_id -> row: built once in O(N), then maintained by every remove / upsert (``add`` drops it).  An index that
        holds an id twice cannot be mutated by id: ``ValueError``."""
        m = self._id_rows
        if m is None:
            m = {d: i for i, d in enumerate(self._doc_ids)}
            if len(m) != len(self._doc_ids):
                seen, twice = set(), []
                for d in self._doc_ids:
                    if d in seen and len(twice) < 5:
                        twice.append(d)
                    seen.add(d)
                raise ValueError(f"the index holds doc ids more than once (e.g. {twice}): remove / upsert need unique ids")
            self._id_rows = m
        return m

    def rows_of(self, doc_ids: Sequence[str]) -> np.ndarray:
        """The row of every given doc id as the index stands now (int64; an unknown id raises ``KeyError``).  Rows change
        with every ``remove``: the tail fills the holes."""
        self._ensure_built()
        ids = [doc_ids] if isinstance(doc_ids, str) else list(doc_ids)
        m = self._row_map()
        missing = [d for d in ids if d not in m]
        if missing:
            raise KeyError(f"unknown doc ids: {sorted(missing, key=str)[:5]}")
        return np.fromiter((m[d] for d in ids), dtype=np.int64, count=len(ids))

    def _corpus_remove(self, rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        return self._corpus.remove_rows(rows)

    def _corpus_put(self, rows: np.ndarray, embeddings, triple) -> None:
        self._corpus.put_rows(rows, embeddings, triple["dewi"], triple["ht_mean"], triple["hi_mean"], normalize=self._normalize)

    def _check_removal(self, n_keep: int) -> None:
        if n_keep <= 0:
            raise ValueError(f"cannot remove every document ({len(self._doc_ids)}): an index keeps at least one")

    def remove(self, doc_ids: Sequence[str]) -> int:
        """Delete documents from the built index in place and return how many (additive; the reference cannot delete).

        Nothing is rebuilt or copied to the host.  Rows are not shifted: with n documents and m of them deleted, the
        surviving documents of the last m rows move into the holes below ``n - m`` (``_engine.plan_remove``), on the device in
        one launch, and ``_doc_ids``, the payloads and ``rows_of`` follow — so row order is no longer insertion order, and
        ``save`` / ``load`` keep the order the index has.  Pending ``add``s are built in first.  Everything is checked before
        any device work, so a failing call leaves the index as it was: an unknown id raises ``KeyError``; an id given twice,
        an index that holds an id twice, or a removal of every document ``ValueError``.  Filters prepared before are refused
        afterwards (``ValueError``), as after a rebuild.  The device storage keeps its size.  The first mutation of an index
        with column-ingested payloads costs O(N) host work (``PayloadStore.follow`` re-gathers the columns into one block
        of its own); later ones O(rows touched)."""
        self._ensure_built()
        ids = [doc_ids] if isinstance(doc_ids, str) else list(doc_ids)
        if len(set(ids)) != len(ids):
            raise ValueError("doc ids to remove must be distinct")
        rows = self.rows_of(ids)
        if not ids:
            return 0
        n_old = len(self._doc_ids)
        self._check_removal(n_old - len(ids))
        self._attr_columns()                        # (a loaded index's attributes go to the device before its rows move)
        src, dst = self._corpus_remove(rows)
        n_keep = n_old - len(ids)
        self._attrs_after_remove(src, dst, n_keep)
        m, all_ids = self._id_rows, self._doc_ids
        for d in ids:
            del m[d]
        for s_, d_ in zip(src.tolist(), dst.tolist()):
            all_ids[d_] = all_ids[s_]
            m[all_ids[d_]] = d_
        del all_ids[n_keep:]
        self._payloads.follow_remove(src, dst, n_old, all_ids, ids, rows)
        self._host_rows = None
        return len(ids)

    def upsert(self, doc_id: str, embedding: np.ndarray, payload: Payload) -> None:
        """Replace the embedding and payload of ``doc_id`` in place, or append it if the index does not hold it (additive)."""
        if embedding.shape != (self.dim,):
            raise ValueError(f"Expected embedding of shape {(self.dim,)}, got {embedding.shape}")
        self.upsert_batch([doc_id], np.asarray(embedding).reshape(1, -1), [payload])

    def upsert_batch(self, doc_ids: Sequence[str], embeddings: np.ndarray, payloads: Sequence[Payload]) -> Tuple[int, int]:
        """``upsert`` of m documents in one launch: returns ``(n_replaced, n_appended)``.  A known id keeps its row; new ids
        are appended in call order at rows ``N, N + 1, ...``.  The stored rows, the bf16 shadow and the payload columns get
        the bits a fresh ``build`` would give them (``dewi_rows_put_f32``).  Checked before any device work like ``remove``
        (an id twice in the call, or held twice: ``ValueError``; shapes: ``add_batch``'s messages)."""
        self._ensure_built()
        emb = np.asarray(embeddings)
        if emb.ndim != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"Expected embeddings of shape (m, {self.dim}), got {emb.shape}")
        if not (len(doc_ids) == emb.shape[0] == len(payloads)):
            raise ValueError("doc_ids, embeddings and payloads must have the same length")
        payloads = list(payloads)
        return self._upsert(list(doc_ids), emb, payload_columns(payloads, ("dewi", "ht_mean", "hi_mean")), payloads, None)

    def upsert_batch_columns(self, doc_ids: Sequence[str], embeddings, columns: Dict[str, np.ndarray]) -> Tuple[int, int]:
        """``upsert_batch`` with the payloads as one array per ``Payload`` field (missing fields are 0.0), as
        ``add_batch_columns`` takes them; ``embeddings`` may be a CUDA fp32 tensor [m, dim] and the columns CUDA tensors."""
        self._ensure_built()
        from . import _native as nat
        shape = tuple(embeddings.shape) if hasattr(embeddings, "shape") else np.shape(embeddings)
        if len(shape) != 2 or int(shape[1]) != self.dim:
            raise ValueError(f"Expected embeddings of shape (m, {self.dim}), got {tuple(shape)}")
        if len(doc_ids) != int(shape[0]):
            raise ValueError("doc_ids and embeddings must have the same length")
        unknown = [name for name in columns if name not in PAYLOAD_FIELDS]
        if unknown:
            raise ValueError(f"unknown payload columns {unknown}")
        m = len(doc_ids)
        cols = {}
        for name in PAYLOAD_FIELDS:
            if name in columns:
                c = columns[name] if nat.is_device_tensor(columns[name]) else np.asarray(columns[name], dtype=np.float64)
                if tuple(c.shape) != (m,):
                    raise ValueError(f"payload column {name!r} has shape {tuple(c.shape)}, expected ({m},)")
                cols[name] = c
        triple = {name: cols.get(name, np.zeros(m, dtype=np.float64)) for name in ("dewi", "ht_mean", "hi_mean")}
        emb = embeddings if nat.is_device_tensor(embeddings) else np.asarray(embeddings)
        return self._upsert(list(doc_ids), emb, triple, None, cols)

    def _upsert(self, ids: List[str], emb, triple, payloads, cols) -> Tuple[int, int]:
        if len(set(ids)) != len(ids):
            raise ValueError("doc ids to upsert must be distinct")
        m = self._row_map()
        if not ids:
            return 0, 0
        n = len(self._doc_ids)
        rows = np.empty(len(ids), dtype=np.int64)
        fresh: List[str] = []
        for i, d in enumerate(ids):
            r = m.get(d)
            if r is None:
                r = n + len(fresh)
                fresh.append(d)
            rows[i] = r
        self._attr_columns()
        self._corpus_put(rows, emb, triple)
        self._attrs_after_put(rows, payloads, cols)
        self._doc_ids.extend(fresh)
        m.update(zip(fresh, range(n, n + len(fresh))))
        self._payloads.follow_put(rows, n, self._doc_ids, ids, objects=payloads, columns=cols)
        self._host_rows = None
        return len(ids) - len(fresh), len(fresh)

    # ---------------------------------------------------------------- build (A2)
    def _raw_matrix(self) -> Tuple[np.ndarray, int]:
        """(all rows as one [N, d] fp32 array, number of leading rows already in stored form)."""
        blocks: List[np.ndarray] = []
        done = 0
        if self._corpus is not None:
            blocks.append(self._stored_rows())
            done = blocks[0].shape[0]
        elif self._loaded_rows is not None:
            blocks.append(self._loaded_rows)
            done = self._loaded_rows.shape[0]
        blocks.extend((b.detach().cpu().numpy() if hasattr(b, "is_cuda") else b).reshape(-1, self.dim) for b in self._pending)
        if not blocks:
            return np.empty((0, self.dim), np.float32), 0
        return (blocks[0] if len(blocks) == 1 else np.concatenate(blocks, axis=0)), done

    def _build_device(self) -> None:
        """``build`` when device-resident blocks are pending: the matrix is assembled (or, for one block that is the
        whole corpus, simply taken) on the GPU, new rows are normalised there, and the two fp32 payload columns the
        re-rank reads are computed on the device.  No row and no column visits the host."""
        import torch
        from . import _native as nat
        from ._engine import DeviceCorpus
        lib = nat.load_library()
        n = len(self._doc_ids)
        dev_blocks = [b for b in self._pending if hasattr(b, "is_cuda")]
        dev = dev_blocks[0].device
        stored = None
        if self._corpus is not None:
            stored = self._corpus.emb.float() if self._corpus.is_bf16 else self._corpus.emb
        elif self._loaded_rows is not None:
            stored = torch.from_numpy(self._loaded_rows).to(dev)
        already = 0 if stored is None else int(stored.shape[0])
        with torch.cuda.device(dev):
            if stored is None and len(self._pending) == 1 and int(dev_blocks[0].shape[0]) == n:
                emb = dev_blocks[0]                                        # the caller's tensor, in place
            else:
                emb = torch.empty((n, self.dim), dtype=torch.float32, device=dev)
                at = 0
                if stored is not None:
                    emb[:already].copy_(stored)
                    at = already
                for b in self._pending:
                    blk = b if hasattr(b, "is_cuda") else torch.from_numpy(np.ascontiguousarray(b.reshape(-1, self.dim), dtype=np.float32))
                    emb[at:at + int(blk.shape[0])].copy_(blk)
                    at += int(blk.shape[0])
                if at != n:
                    raise ValueError(f"{n} doc ids but {at} embedding rows")
            if self._normalize and already < n:
                tail = emb[already:]
                nat.check(lib.dewi_normalize_rows_f32(nat.ptr(tail), nat.ptr(tail), n - already, self.dim, nat.stream_ptr()))
            # payload columns: device blocks contribute on the device; rows that came with host data through the host
            fields = ("dewi", "ht_mean", "hi_mean")
            blocks = list(self._payloads.column_blocks())
            covered = sum(r1 - r0 for r0, r1, cols, made in blocks
                          if any(hasattr(c, "is_cuda") for c in cols.values()) and not made)
            if covered == n:
                c64 = {}
                for name in fields:
                    # (a block may mix CUDA and host columns: PayloadStore keeps host ones as ndarrays — as_tensor takes both)
                    parts = [(torch.as_tensor(cols[name]).to(device=dev, dtype=torch.float64) if name in cols
                              else torch.zeros(r1 - r0, dtype=torch.float64, device=dev)) for r0, r1, cols, _ in blocks]
                    c64[name] = (parts[0] if len(parts) == 1 else torch.cat(parts)).contiguous()
            else:
                host = self._payload_columns()
                c64 = {name: torch.from_numpy(host[name]).to(dev) for name in fields}
            dewi32 = torch.empty(n, dtype=torch.float32, device=dev)
            ent32 = torch.empty(n, dtype=torch.float32, device=dev)
            nat.check(lib.dewi_payload_soa_f64(nat.ptr(c64["dewi"]), nat.ptr(c64["ht_mean"]), nat.ptr(c64["hi_mean"]),
                                               nat.ptr(dewi32), nat.ptr(ent32), n, nat.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        self._corpus = DeviceCorpus(emb, dewi32, ent32, self.space)
        if self._batch_shadow and self.space == "cosine":
            self._corpus.enable_bf16_shadow(single_query=self._shadow_single)
        if self._int8_shadow:
            self._corpus.enable_int8_shadow()
        if self._binary_shadow:
            self._corpus.enable_binary_shadow()
        self._pending = []
        self._pending_rows = 0
        self._loaded_rows = None
        self._host_rows = None
        self._is_trained = True

    def build(self, **kwargs: Any) -> None:
        from ._engine import DeviceCorpus
        if any(hasattr(b, "is_cuda") for b in self._pending):
            return self._build_device()
        rows, already = self._raw_matrix()
        if rows.shape[0] == 0:
            raise ValueError("No embeddings to build index from")
        if rows.shape[0] != len(self._doc_ids):
            raise ValueError(f"{len(self._doc_ids)} doc ids but {rows.shape[0]} embedding rows")
        cols = self._payload_columns()
        if already == 0 or not self._normalize:
            corpus = DeviceCorpus.from_host(rows, cols["dewi"], cols["ht_mean"], cols["hi_mean"], self.space,
                                            normalize=self._normalize, device=self._device)
        else:
            # rows [0, already) are stored (normalised) rows: normalise only the new tail
            head = DeviceCorpus.from_host(rows, cols["dewi"], cols["ht_mean"], cols["hi_mean"], self.space,
                                          normalize=False, device=self._device)
            if already < rows.shape[0]:
                import torch
                from . import _native as nat
                tail = head.emb[already:]
                with torch.cuda.device(head.device):       # the kernel goes on THAT device's current stream
                    nat.check(nat.load_library().dewi_normalize_rows_f32(nat.ptr(tail), nat.ptr(tail),
                                                                         rows.shape[0] - already, self.dim,
                                                                         nat.stream_ptr()))
                    torch.cuda.current_stream().synchronize()
            corpus = head
        self._corpus = (corpus.enable_bf16_shadow(single_query=self._shadow_single)
                        if self._batch_shadow and self.space == "cosine" else corpus)
        if self._int8_shadow:
            self._corpus.enable_int8_shadow()
        if self._binary_shadow:
            self._corpus.enable_binary_shadow()
        self._pending = []
        self._pending_rows = 0
        self._loaded_rows = None
        self._host_rows = None
        self._is_trained = True

    def _payload_columns(self, fields: Tuple[str, ...] = ("dewi", "ht_mean", "hi_mean")) -> Dict[str, np.ndarray]:
        """float64 ``dewi`` / ``ht_mean`` / ``hi_mean`` (or other ``Payload`` ``fields``) of every row, in row order.  Column-ingested
        blocks are copied as arrays (objects already handed out for some of their rows win, so in-place
        edits of a returned ``Payload`` are seen by ``refresh_payloads``); the rest is read from objects."""
        n = len(self._doc_ids)
        store = self._payloads
        out = {name: np.zeros(n, dtype=np.float64) for name in fields}
        covered = np.zeros(n, dtype=bool)
        for row0, row1, cols, made in store.column_blocks():
            for name in fields:
                if name in cols:
                    c = cols[name]
                    out[name][row0:row1] = c.detach().cpu().numpy() if hasattr(c, "is_cuda") else c
            for row, p in made.items():
                for name in fields:
                    out[name][row] = getattr(p, name)
            covered[row0:row1] = True
        if not covered.all():
            rows = np.nonzero(~covered)[0]
            plist = [dict.__getitem__(store, self._doc_ids[r]) for r in rows.tolist()]
            sub = payload_columns(plist, fields)
            for name in fields:
                out[name][rows] = sub[name]
        return out

    def refresh_payloads(self) -> None:
        """Re-snapshot ``dewi`` / ``ht_mean`` / ``hi_mean`` of every Payload into the HBM columns."""
        if self._corpus is None:
            return
        import torch
        from . import _native as nat
        cols = self._payload_columns()
        dev = self._corpus.device
        with torch.cuda.device(dev):                       # the kernel goes on THAT device's current stream
            d = [torch.from_numpy(cols[k]).to(dev) for k in ("dewi", "ht_mean", "hi_mean")]
            nat.check(nat.load_library().dewi_payload_soa_f64(nat.ptr(d[0]), nat.ptr(d[1]), nat.ptr(d[2]),
                                                              nat.ptr(self._corpus.dewi32), nat.ptr(self._corpus.ent32),
                                                              len(self._doc_ids), nat.stream_ptr()))
            torch.cuda.current_stream().synchronize()

    # ---------------------------------------------------------------- stored rows on the host
    def _stored_rows(self) -> np.ndarray:
        if self._host_rows is None:
            self._host_rows = self._corpus.emb.float().cpu().numpy()
        return self._host_rows

    @property
    def _embeddings(self):
        """What the reference keeps in ``_embeddings``: a list of rows before ``build``, the N x d
        fp32 matrix after (index.py:101-116 reaches into it).  Materialised from HBM on demand."""
        if self._corpus is not None and not self._pending:
            return self._stored_rows()
        if self._corpus is None and self._loaded_rows is not None and not self._pending:
            return self._loaded_rows
        rows, _ = self._raw_matrix()
        return [r for r in rows]

    @_embeddings.setter
    def _embeddings(self, value) -> None:
        arr = np.asarray(value, dtype=np.float32)
        self._corpus = None
        self._pending = []
        self._pending_rows = 0
        self._loaded_rows = arr.reshape(-1, self.dim) if arr.size else None
        self._invalidate()

    # ---------------------------------------------------------------- search (A3 + A4)
    def _ensure_built(self) -> None:
        if self._corpus is None or self._pending or not self._is_trained:
            self.build()

    # ---------------------------------------------------------------- filters (additive)
    def filter_mask(self, mask=None, *, doc_ids: Optional[Sequence[str]] = None, rows=None):
        """The bool row mask of exactly one of: ``mask`` (bool array of length N, numpy or torch, host or device: returned
        as it is after the checks), ``doc_ids`` (through this index's ids; an unknown id raises ``KeyError``) or ``rows``
        (integer row positions, 0 <= row < N).  Host logic only: no device work."""
        given = [x is not None for x in (mask, doc_ids, rows)]
        if sum(given) != 1:
            raise ValueError("pass exactly one of mask, doc_ids, rows")
        n = len(self._doc_ids)
        if mask is not None:
            shape = tuple(mask.shape) if hasattr(mask, "shape") else (len(mask),)
            if shape != (n,):
                raise ValueError(f"filter mask must have shape ({n},), got {shape}")
            if hasattr(mask, "is_cuda"):
                import torch
                if mask.dtype != torch.bool:
                    raise ValueError(f"filter mask must be boolean, got {mask.dtype}")
                return mask
            m = np.asarray(mask)
            if m.dtype != np.bool_:
                raise ValueError(f"filter mask must be boolean, got {m.dtype}")
            return m
        if doc_ids is not None:
            if isinstance(doc_ids, str):
                doc_ids = [doc_ids]
            wanted = set(doc_ids)
            hit = np.fromiter((d in wanted for d in self._doc_ids), dtype=bool, count=n)
            missing = wanted.difference(np.asarray(self._doc_ids, dtype=object)[hit].tolist()) if wanted else set()
            if missing:
                raise KeyError(f"unknown doc ids: {sorted(missing, key=str)[:5]}")
            return hit
        r = rows.detach().cpu().numpy() if hasattr(rows, "is_cuda") else np.asarray(rows)
        r = r.reshape(-1)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError(f"filter rows must be integers, got {r.dtype}")
        if r.size and (int(r.min()) < 0 or int(r.max()) >= n):
            raise ValueError(f"filter rows must lie in [0, {n})")
        out = np.zeros(n, dtype=bool)
        out[r.astype(np.int64)] = True
        return out

    def make_filter(self, mask=None, *, doc_ids: Optional[Sequence[str]] = None, rows=None):
        """Prepare an allow-list for ``search`` / ``search_batch(filter=...)`` (additive): one of a bool ``mask`` of
        length N, ``doc_ids`` or row positions ``rows`` (see ``filter_mask``).  The result is a ``DeviceFilter`` bound
        to the index as it is built now: after ``add`` + ``build`` (or on another index, ``load`` included) it raises
        ``ValueError`` instead of answering from stale rows."""
        self._ensure_built()
        return self._corpus.make_filter(self.filter_mask(mask, doc_ids=doc_ids, rows=rows))

    def query_filter_masks(self, masks=None, *, doc_ids=None, rows=None):
        """The bool [B, N] masks of exactly one of: ``masks`` (bool array of shape [B, N], numpy or torch, host or device:
        returned as it is after the checks), ``doc_ids`` (B sequences of doc ids) or ``rows`` (B integer row arrays).
        Every row goes through the checks of ``filter_mask``.  Host logic only: no device work."""
        given = [x is not None for x in (masks, doc_ids, rows)]
        if sum(given) != 1:
            raise ValueError("pass exactly one of masks, doc_ids, rows")
        n = len(self._doc_ids)
        if masks is not None:
            shape = tuple(masks.shape) if hasattr(masks, "shape") else tuple(np.shape(masks))
            if len(shape) != 2 or shape[0] < 1:
                raise ValueError(f"query filter masks must have shape (B, {n}) with B >= 1, got {shape}")
            if hasattr(masks, "is_cuda"):
                for j in range(shape[0]):
                    self.filter_mask(masks[j])
                return masks
            return np.stack([self.filter_mask(np.asarray(masks[j])) for j in range(shape[0])])
        lists = list(doc_ids if doc_ids is not None else rows)
        if not lists:
            raise ValueError("query filters need at least one list")
        if doc_ids is not None:
            return np.stack([self.filter_mask(doc_ids=[d] if isinstance(d, str) else list(d)) for d in lists])
        return np.stack([self.filter_mask(rows=r) for r in lists])

    def make_query_filters(self, masks=None, *, doc_ids=None, rows=None):
        """Prepare one allow-list per query for ``search_batch(filter=...)`` (additive): exactly one of a bool ``masks``
        array of shape [B, N], ``doc_ids`` (B sequences of doc ids) or ``rows`` (B integer row arrays), see
        ``query_filter_masks``.  Query j of a batch of B then searches only its own list.  The result is a
        ``DeviceQueryFilters`` bound to the index as it is built now (stale-checked like ``make_filter``)."""
        self._ensure_built()
        return self._corpus.make_query_filters(self.query_filter_masks(masks, doc_ids=doc_ids, rows=rows))

    def _prepared(self, filter):
        """A ``DeviceFilter`` / ``DeviceQueryFilters``, a ``Where`` predicate over the attribute columns (a list of B of them:
        one per query), anything ``make_filter`` takes (bool mask, doc ids, integer rows) or a bool [B, N] mask
        (``make_query_filters``), prepared on the fly."""
        from ._engine import DeviceFilter, DeviceQueryFilters
        if isinstance(filter, Where):
            return self.make_filter_where(filter)
        if is_where_list(filter):
            return self.make_query_filters_where(filter)
        if filter is None or isinstance(filter, (DeviceFilter, DeviceQueryFilters)):
            return filter
        if len(getattr(filter, "shape", ())) == 2:
            return self.make_query_filters(filter)
        return self.make_filter(**filter_kwargs(filter))

    #: largest batch ``approx=None`` sends through the int8 route.  Set when the route scanned the corpus once per FOUR queries
    #: and lost to the exact matrix-core batch beyond (1 M x 768, k = 10: 4 queries 0.34 ms against 0.50 exact, 32 queries
    #: 2.58 ms against 0.55 — DESIGN.md 4.1q).  Larger batches now take the int8 matrix-core pass when they ARE
    #: sent (``approx=True``); the default stays: raising it would change what existing calls return.
    APPROX_AUTO_MAX_BATCH = 4

    def _use_approx(self, approx: Optional[bool], similarity: str, filter, k: int, candidates: Optional[int],
                    n_queries: int = 1) -> bool:
        """Whether a search takes the int8 route.  ``approx=True``: it must (``ValueError`` without an int8 shadow, with a
        ``filter`` or with a similarity transform); ``None``: it does where the index has an int8 shadow and the route
        serves the call (no filter, no transform, a cut of at most 1024, at most ``APPROX_AUTO_MAX_BATCH`` queries);
        ``False``: never."""
        if approx is None:
            if not self._int8_shadow or filter is not None or similarity != "ip" or int(n_queries) > self.APPROX_AUTO_MAX_BATCH:
                return False
            from . import _native as nat
            return (2 * int(k) if candidates is None else int(candidates)) <= nat.I8_MAX_CANDIDATES
        if not approx:
            return False
        if not self._int8_shadow:
            raise ValueError("approx=True needs an index built with int8_shadow=True")
        if filter is not None:
            raise ValueError("approx=True does not take a filter: filtered searches run on the fp32 rows (approx=False); "
                             "the int8 route over an allow-list is search_approx_filtered")
        if similarity != "ip":
            raise ValueError("approx=True does not take a similarity transform")
        return True

    def search(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
               candidates: Optional[int] = None, similarity: str = "ip", *, approx: Optional[bool] = None,
               rescore: bool = True, filter=None) -> SearchResult:
        """Reference ``ExactIndex.search`` (backends.py:414-481) for one query.

        ``candidates`` (additive): how many nearest rows are re-ranked.  Default ``min(2k, N)``, the
        reference's ExactIndex rule; ``candidates=k`` is the rule of its HNSW / FAISS backends
        (backends.py:217-240, 326-356: exactly k neighbours are blended and sorted) on exact neighbours,
        with ``similarity`` choosing what those backends blend: "ip" (faiss inner product, :335-336),
        "one_minus_dist" (hnswlib ``1 - dist``, :229-231) or "inv_one_plus_dist" (faiss L2
        ``1/(1+dist)``, :337-338).  hnswlib / faiss are not installed here: that rule is restated by
        reading and its parity is unpinned.

        ``filter`` (additive): restrict the search to an allow-list — a prepared filter (``make_filter``) or anything
        ``make_filter`` takes.  The result is the reference's search applied to the allowed rows only: c = min(2k, |A|),
        ``[]`` for an empty filter, ``ValueError`` for k > |A|.  Per-query filters (``make_query_filters``) of one query
        are accepted as well.

        ``approx`` / ``rescore`` (additive, keyword-only like ``filter``): see ``search_batch``.
        """
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores = self.search_batch(q, k, eta, entropy_pref, candidates, similarity, approx=approx, rescore=rescore,
                                         filter=filter)
        keep = rows[:1] >= 0            # (per-query filters: an empty list pads its row with id -1)
        return self.results_for(rows[:1][:, keep[0]], scores[:1][:, keep[0]])[0]

    def search_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                     candidates: Optional[int] = None, similarity: str = "ip", *, approx: Optional[bool] = None,
                     rescore: bool = True, filter=None) -> Tuple[np.ndarray, np.ndarray]:
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k]).  ``filter``: see ``search``
        (one allow-list for every query of the batch; [B, 0] results when it is empty or k <= 0).  Per-query filters —
        a ``DeviceQueryFilters`` of B lists (``make_query_filters``) or a bool [B, N] mask — restrict query j to its own
        list F_j, with the rules of one list per query (c = min(2k, |F_j|), ``ValueError`` naming the query for
        k > |F_j| > 0); the row of a query whose list is empty is padded with id -1 and score NaN.

        ``approx`` (additive; an index built with ``int8_shadow=True``): take the candidate cut — ``min(2k, N)``, or
        ``candidates`` up to 1024 — by the INT8 scores of the shadow (a quarter of the bytes of the fp32 rows), re-score it
        from the fp32 rows (``rescore=True``; ``False`` blends the int8 scores as they are) and finish as ever.  Approximate:
        a document is missed when the int8 scores drop it from the cut (measured recall: DESIGN.md 4.1q).  ``None`` (default)
        means "the index has an int8 shadow" — where the route serves the call (no filter, no similarity transform, a cut
        of at most 1024, at most ``APPROX_AUTO_MAX_BATCH`` = 4 queries; ``approx=True`` takes it for any batch — from 2
        queries on through the int8 matrix-core pass, 32 queries per read of the codes, with the same results bit for bit:
        DESIGN.md 4.1x); ``True`` without a shadow, with ``filter=`` or with a transform raises ``ValueError``; ``False`` is
        the exact path, bit for bit.  After ``remove`` / ``upsert*`` the next approximate search re-quantises the whole
        matrix (one pass over the fp32 rows), so a mutated index answers as a freshly built one."""
        use_approx = self._use_approx(approx, similarity, filter, k, candidates,      # (argument errors before any build)
                                      np.shape(queries)[0] if np.ndim(queries) == 2 else 1)
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if use_approx:
            return self._corpus.search_approx(q, int(k), float(eta), float(entropy_pref), candidates=candidates,
                                              rescore=bool(rescore))
        if filter is not None:
            return self._corpus.search(q, int(k), float(eta), float(entropy_pref), candidates=candidates,
                                       similarity=similarity, filter=self._prepared(filter))
        return self._corpus.search(q, int(k), float(eta), float(entropy_pref), candidates=candidates,
                                   similarity=similarity)

    # ---------------------------------------------------------------- approximate search over the binary copy (additive)
    def search_binary(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *,
                      candidates: Optional[int] = None, rescore: bool = True) -> SearchResult:
        """``search`` over the 1-bit copy (an index built with ``binary_shadow=True``): see ``search_binary_batch``."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores = self.search_binary_batch(q[:1], k, eta, entropy_pref, candidates=candidates, rescore=rescore)
        return self.results_for(rows[:1], scores[:1])[0]

    def search_binary_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *,
                            candidates: Optional[int] = None, rescore: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k]) with the candidate cut taken by HAMMING
        distance between the sign bits of the query and of the stored rows: one bit per element, 1 / 32 of the fp32 rows'
        bytes.  The cut is ``min(N, 1024, max(128, 16 k))`` or ``candidates`` (up to 1024); ``rescore=True`` re-scores it from
        the fp32 rows and blends as every search, ``False`` blends the Hamming similarity ``(dim - 2 h) / dim``.
        Approximate: a document is missed when the Hamming scores drop it from the cut (measured recall: DESIGN.md 4.1aa).
        Cosine, ``dim % 128 == 0`` from 128 to 4096; no filter, no similarity transform; nothing routes here by itself
        (``search`` and its ``approx=`` mean what they meant).  ``ValueError``: no binary shadow, ``k`` above the cut, a cut
        above 1024.  After ``remove`` / ``upsert*`` the next binary search re-binarises the whole matrix."""
        if not self._binary_shadow:
            raise ValueError("search_binary needs an index built with binary_shadow=True")
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        return self._corpus.search_binary(q, int(k), float(eta), float(entropy_pref), candidates=candidates,
                                          rescore=bool(rescore))

    # ---------------------------------------------------------------- approximate search over an allow-list (additive)
    def search_approx_filtered(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                               candidates: Optional[int] = None, *, filter, rescore: bool = True) -> SearchResult:
        """``search(filter=...)`` on the int8 route (an index built with ``int8_shadow=True``): see
        ``search_approx_filtered_batch``."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores = self.search_approx_filtered_batch(q[:1], k, eta, entropy_pref, candidates, filter=filter, rescore=rescore)
        keep = rows[0] >= 0
        return self.results_for(rows[:1][:, keep], scores[:1][:, keep])[0]

    def search_approx_filtered_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                                     candidates: Optional[int] = None, *, filter,
                                     rescore: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k]) over the rows of ``filter`` — whatever
        ``search_batch(filter=)`` accepts, a ``dedup_filter(...)`` and per-query filters included — with the candidate cut
        (``min(2k, |A|)``, or ``candidates`` up to 1024) taken by the INT8 scores of the listed rows: a quarter of the bytes
        the exact filtered search reads.  ``rescore=True`` re-scores the cut from the fp32 rows; ``False`` blends the int8
        scores.  Approximate in the way ``search_batch(approx=True)`` is.  ``ValueError``: no int8 shadow, a stale filter,
        ``k`` above ``|A|``; an empty filter gives [B, 0], an empty list of per-query filters pads its row with -1 / NaN."""
        if not self._int8_shadow:
            raise ValueError("search_approx_filtered needs an index built with int8_shadow=True")
        if filter is None:
            raise ValueError("search_approx_filtered needs a filter (search(approx=True) is the unfiltered route)")
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        return self._corpus.search_approx_filtered(q, int(k), float(eta), float(entropy_pref), filter=self._prepared(filter),
                                                   candidates=candidates, rescore=bool(rescore))

    # ---------------------------------------------------------------- diverse search (additive)
    def search_diverse(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                       mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                       max_sim: Optional[float] = None) -> SearchResult:
        """``search`` with a per-query guard against near-duplicates (additive; the reference has no such method): maximal
        marginal relevance (Carbonell & Goldstein 1998) over the query's ``candidates`` most similar documents (default
        ``4k``, at most 1024).  Results are picked one by one, each the candidate with the largest ``mmr_lambda * adjusted
        score - (1 - mmr_lambda) * (largest similarity to a document already picked)``; a candidate at least ``max_sim``
        similar to a picked document is struck out, so the answer may be shorter than k.  Returns ``(doc_id, adjusted score,
        Payload)`` tuples like ``search``, here IN PICK ORDER.  ``mmr_lambda=1.0, max_sim=0.95`` is the plain ranking of the
        pool with every later copy of an earlier result removed; ``mmr_lambda=1.0`` alone is ``search(candidates=...)``.
        Cosine indexes (``space="l2"``: ``NotImplementedError``); no ``filter`` in this build."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores = self.search_diverse_batch(q[:1], k, eta, entropy_pref, mmr_lambda, candidates, max_sim)
        keep = rows[0] >= 0             # (fewer than k eligible documents: the tail is padded with id -1)
        return self.results_for(rows[:1][:, keep], scores[:1][:, keep])[0]

    def search_diverse_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                             mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                             max_sim: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k]) in pick order; a query with fewer
        than k eligible documents pads its row with id -1 and score NaN, as per-query filters do.  See ``search_diverse``."""
        if self.space == "l2":
            raise NotImplementedError("diverse search penalises the inner product of unit rows: space='l2' is not in this build")
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        return self._corpus.search_diverse(q, int(k), float(eta), float(entropy_pref), float(mmr_lambda), candidates, max_sim)

    # ---------------------------------------------------------------- subset selection (additive)
    def select_subset(self, budget: int, mmr_lambda: float = 0.5, max_sim: Optional[float] = None, relevance=None,
                      filter=None, seeds: Optional[Sequence[str]] = None, return_gain: bool = False,
                      return_coverage: bool = False):
        """The ``budget`` most informative documents that do not repeat each other (additive; the reference measures such a
        selection — ``metrics.cluster_coverage`` — but cannot make one): greedy maximal marginal relevance over the WHOLE
        corpus.  Each pick is the document with the largest ``mmr_lambda * relevance - (1 - mmr_lambda) * (largest similarity
        to a document already picked)``; a document at least ``max_sim`` similar to a picked one is struck out, so the answer
        may be shorter than ``budget`` (a budget above N returns at most N).  ``relevance``: N values, an array or a CUDA
        tensor (default: the ``dewi`` column as built; NaN: never picked).  ``filter``: what ``search(filter=)`` takes for one
        list — only its documents can be picked (and only they are penalised).  ``seeds``: doc ids already chosen elsewhere:
        they penalise, are not returned and do not count.

        Returns the doc ids IN PICK ORDER; with ``return_gain`` also their marginal values at the pick (fp32 array); with
        ``return_coverage`` also, per document of the index, the nearest selected doc id (``None``: none) and its similarity
        (NaN: none; for a struck-out document as it stood when it was struck out).  ``make_filter(doc_ids=
        index.select_subset(...))`` is the allow-list of the subset.  One corpus pass per pick: thousands of picks over a
        million documents take seconds; ``select_subset_blocked`` gives the same answer with many picks per pass.
        Cosine indexes (``space="l2"``: ``NotImplementedError``)."""
        return self._select_subset(budget, mmr_lambda, max_sim, relevance, filter, seeds, return_gain, return_coverage, None)

    def select_subset_blocked(self, budget: int, mmr_lambda: float = 0.5, max_sim: Optional[float] = None, relevance=None,
                              filter=None, seeds: Optional[Sequence[str]] = None, return_gain: bool = False,
                              return_coverage: bool = False, picks_per_pass: Optional[int] = 32):
        """``select_subset`` in the BLOCKED form: the same answer bit for bit — an exact batched greedy, not a lazy or
        stochastic one — with up to ``picks_per_pass`` picks applied by one corpus pass (clipped to what the row shape
        takes; ``None`` / 1: the one-pick form; ``DeviceCorpus.select_subset_device``).  For budgets of a real fraction of
        the corpus and for many ``seeds``.  One host synchronisation per chunk of rounds.  A method of its own: the parameter
        list of ``select_subset`` is fixed."""
        return self._select_subset(budget, mmr_lambda, max_sim, relevance, filter, seeds, return_gain, return_coverage,
                                   picks_per_pass)

    def select_subset_grouped(self, budget: int, *, groups, per_group: int = 1, quotas=None, mmr_lambda: float = 0.5,
                              max_sim: Optional[float] = None, relevance=None, filter=None, seeds: Optional[Sequence[str]] = None,
                              seeds_count: bool = True, return_gain: bool = False, return_coverage: bool = False,
                              picks_per_pass: Optional[int] = 32):
        """``select_subset`` with GROUP QUOTAS: at most ``per_group`` picks from one group — "10 000 documents, at most 50 per
        site" (additive; the selection side of ``search_collapsed``).  It is the greedy run itself that respects the quota: a
        group that is full is struck out, so the budget it would have taken goes to other groups and its documents stop
        penalising nobody they did not penalise already — selecting too many and pruning afterwards is a different subset.
        ``groups``: anything ``make_groups`` takes, or a prepared ``DeviceGroups`` (stale-checked); ungrouped documents are free
        of any quota.  ``quotas``: a mapping from group value to that group's quota; it overrides ``per_group`` (<= 0: nothing
        from that group).  ``seeds_count``: each seed lowers its group's quota by one.  ``picks_per_pass``: ``None`` / 1 takes
        the one-pick form, otherwise as in ``select_subset_blocked``; the answer is the same bit for bit.  Everything else,
        and the return values, as ``select_subset``."""
        if self.space == "l2":
            raise NotImplementedError("subset selection penalises the inner product of unit rows: space='l2' is not in this build")
        if int(per_group) <= 0:
            raise ValueError(f"per_group must be at least 1, got {per_group}")
        from ._engine import DeviceGroups, dense_group_labels
        self._ensure_built()
        if isinstance(groups, DeviceGroups):
            self._corpus.check_groups(groups)
        is_mapping = hasattr(groups, "keys") and not hasattr(groups, "dtype")
        dense, codes = dense_group_labels(groups, len(self._doc_ids), self._row_map() if is_mapping else None)
        return self._select_subset(budget, mmr_lambda, max_sim, relevance, filter, seeds, return_gain, return_coverage,
                                   picks_per_pass, (dense, codes, int(per_group), quotas, bool(seeds_count)))

    def _select_subset(self, budget, mmr_lambda, max_sim, relevance, filter, seeds, return_gain, return_coverage, picks_per_pass,
                       grouped=None):
        if self.space == "l2":
            raise NotImplementedError("subset selection penalises the inner product of unit rows: space='l2' is not in this build")
        self._ensure_built()
        import torch
        from ._engine import DeviceFilter, DeviceQueryFilters
        corpus = self._corpus
        n = len(self._doc_ids)
        with corpus._lock, torch.cuda.device(corpus.device):
            mask = None
            if isinstance(filter, Where):
                filter = self.make_filter_where(filter)
            if isinstance(filter, DeviceQueryFilters) or is_where_list(filter):
                raise ValueError("select_subset takes one allow-list, not per-query filters")
            if isinstance(filter, DeviceFilter):
                corpus.check_filter(filter)
                mask = filter.byte_mask()
            elif filter is not None:
                m = self.filter_mask(**filter_kwargs(filter))
                mask = (m if hasattr(m, "is_cuda") else torch.from_numpy(np.ascontiguousarray(m))).to(corpus.device)
            rel = None
            if relevance is not None:
                r = relevance if hasattr(relevance, "is_cuda") else torch.from_numpy(
                    np.ascontiguousarray(np.asarray(relevance, dtype=np.float32)))
                if tuple(r.shape) != (n,):
                    raise ValueError(f"relevance must have shape ({n},), got {tuple(r.shape)}")
                rel = r.to(device=corpus.device, dtype=torch.float32)
            seed_rows = None
            if seeds is not None:
                seed_rows = self.rows_of([seeds] if isinstance(seeds, str) else list(seeds))
            group_kw = {}
            if grouped is not None:
                from ._engine import grouped_quotas
                dense, codes, per_group, quotas, seeds_count = grouped
                in_range = [r for r in np.asarray(seed_rows if seed_rows is not None else [], np.int64).reshape(-1).tolist()
                            if 0 <= r < n]
                q = grouped_quotas(codes, per_group, quotas, dense[in_range] if seeds_count else ())
                if q is not None and q.size == 0:
                    q = None                       # nobody is grouped: one group that nobody belongs to
                group_kw = dict(group_labels=torch.from_numpy(dense).to(corpus.device), n_groups=max(len(codes), 1),
                                per_group=per_group, group_quota=None if q is None else torch.from_numpy(q).to(corpus.device))
            out = corpus.select_subset_device(int(budget), float(mmr_lambda), max_sim, rel, mask, seed_rows,
                                              return_coverage=bool(return_coverage), picks_per_pass=picks_per_pass, **group_kw)
            kk = int(out[2].item())
            rows = out[0][:kk].cpu().numpy() - corpus.id_offset
            result = [[self._doc_ids[r] for r in rows.tolist()]]
            if return_gain:
                result.append(out[1][:kk].cpu().numpy())
            if return_coverage:
                owner = out[4].cpu().numpy()
                result.append([self._doc_ids[o - corpus.id_offset] if o >= 0 else None for o in owner.tolist()])
                result.append(out[3].cpu().numpy())
        return result[0] if len(result) == 1 else tuple(result)

    def search_diverse_approx(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                              mmr_lambda: float = 0.5, candidates: Optional[int] = None, max_sim: Optional[float] = None,
                              rescore: bool = True) -> SearchResult:
        """``search_diverse`` with the pool taken by the int8 scores of the shadow and — ``rescore=True`` — re-scored from the
        fp32 rows (an index built with ``int8_shadow=True``; ``ValueError`` otherwise).  A method of its own: the parameter
        lists of ``search_diverse`` / ``search_diverse_batch`` are fixed."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores = self.search_diverse_approx_batch(q[:1], k, eta, entropy_pref, mmr_lambda, candidates, max_sim, rescore)
        keep = rows[0] >= 0
        return self.results_for(rows[:1][:, keep], scores[:1][:, keep])[0]

    def search_diverse_approx_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                                    mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                                    max_sim: Optional[float] = None, rescore: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k]) in pick order, padded with id -1 /
        score NaN: ``search_diverse_batch`` over the int8 route's pool.  See ``search_diverse_approx``."""
        if not self._int8_shadow:
            raise ValueError("an approximate diverse search needs an index built with int8_shadow=True")
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        return self._corpus.search_diverse_approx(q, int(k), float(eta), float(entropy_pref), float(mmr_lambda), candidates,
                                                  max_sim, bool(rescore))

    # ---------------------------------------------------------------- collapsed search (additive)
    def make_groups(self, groups):
        """Prepare group labels for ``search_collapsed`` / ``search_collapsed_batch`` (additive).  ``groups`` is one of: a
        ``DuplicateGroups`` (its ``labels``); an integer array [N] in row order, negative meaning ungrouped; a sequence of N
        hashables in row order (source site, album, author, ...; ``None``: ungrouped), factorised on the host; a mapping
        ``doc_id -> hashable`` (documents not named are ungrouped; an unknown doc id raises ``KeyError``).  A wrong length or
        integer labels outside int32 raise ``ValueError``.  The result is a ``DeviceGroups`` bound to the index as it is built
        now: after a rebuild, ``remove`` or ``upsert*`` it raises ``ValueError`` instead of folding the wrong rows."""
        from ._engine import DeviceGroups, group_labels
        self._ensure_built()
        if isinstance(groups, DeviceGroups):
            self._corpus.check_groups(groups)
            return groups
        is_mapping = hasattr(groups, "keys") and not hasattr(groups, "dtype")
        lab, _ = group_labels(groups, len(self._doc_ids), self._row_map() if is_mapping else None)
        return self._corpus.make_groups(lab)

    def search_collapsed(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *, groups,
                         per_group: int = 1, candidates: Optional[int] = None, filter=None, approx: bool = False,
                         rescore: bool = True, widen: bool = False, return_hits: bool = False):
        """``search`` with at most ``per_group`` results from one group (additive; the reference has no such method; search
        engines call it field collapsing): the k best documents of the query's pool — its ``candidates`` most similar
        documents, default ``4k``, at most 2048 — in ``search`` order, a document being dropped when ``per_group`` documents of
        its group rank before it.  ``groups``: anything ``make_groups`` takes, or a prepared ``DeviceGroups``.  Unlike
        ``dedup_filter`` the member that stands for a group is the best one FOR THIS QUERY, and a group need not be geometric.

        ``filter``: whatever ``search(filter=)`` takes for ONE allow-list (a mask, doc ids, rows, a prepared filter,
        ``dedup_filter(...)``); per-query filters raise ``NotImplementedError``.  ``approx=True`` (an index with the int8
        shadow) takes the pool by the int8 scores (at most 1024), re-scored from the fp32 rows unless ``rescore=False``.
        ``widen=True`` runs a query again with four times the pool while it has fewer than k results and the pool can still
        grow (cap 2048, N, or the filter's rows); a query still short at the cap returns fewer than k results — for groups
        larger than the cap fold them corpus-wide with ``dedup_filter`` instead.

        Returns ``(doc_id, adjusted score, Payload)`` tuples like ``search``; with ``return_hits=True`` ``(results, hits)``,
        ``hits[i]`` the number of documents of the pool in result i's group (1 for an ungrouped document): "+37 similar"."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores, hits = self.search_collapsed_batch(q[:1], k, eta, entropy_pref, groups=groups, per_group=per_group,
                                                         candidates=candidates, filter=filter, approx=approx, rescore=rescore,
                                                         widen=widen, return_hits=True)
        keep = rows[0] >= 0             # (fewer than k results: the tail is padded with id -1)
        res = self.results_for(rows[:1][:, keep], scores[:1][:, keep])[0]
        return (res, hits[0][keep].tolist()) if return_hits else res

    def search_collapsed_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *, groups,
                               per_group: int = 1, candidates: Optional[int] = None, filter=None, approx: bool = False,
                               rescore: bool = True, widen: bool = False, return_hits: bool = False, return_pool: bool = False):
        """[B, dim] queries -> ``(row indices int64 [B, k], adjusted scores fp32 [B, k])``, with ``return_hits=True`` also
        ``hits`` int32 [B, k], with ``return_pool=True`` also each query's final pool size int64 [B]; a query with fewer than
        k results pads its row with -1 / NaN / 0.  See ``search_collapsed``."""
        from ._engine import DeviceQueryFilters
        if int(per_group) <= 0:
            raise ValueError(f"per_group must be positive, got {per_group}")
        if isinstance(filter, DeviceQueryFilters) or is_where_list(filter) or (filter is not None and len(getattr(filter, "shape", ())) == 2):
            raise NotImplementedError("a collapsed search takes one allow-list for the batch (per-query filters: not in this build)")
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        corpus = self._corpus
        if approx and not corpus.has_int8_shadow:
            raise ValueError("approx=True needs an index built with its int8 copy (int8_shadow=True)")
        if filter is not None and corpus.is_bf16:
            raise NotImplementedError("filtered search serves fp32 corpora (bf16: not in this build)")
        out = corpus.search_collapsed(q, int(k), float(eta), float(entropy_pref), groups=self.make_groups(groups),
                                      per_group=int(per_group), candidates=candidates, filter=self._prepared(filter),
                                      approx=bool(approx), rescore=bool(rescore), widen=bool(widen), return_pool=True)
        rows, scores, hits, pool = out
        if corpus.id_offset:
            rows = np.where(rows >= 0, rows - corpus.id_offset, rows)
        res = (rows, scores)
        if return_hits:
            res += (hits,)
        if return_pool:
            res += (pool,)
        return res

    # ---------------------------------------------------------------- search by examples (additive)
    def _example_parts(self, positive, negative):
        """``positive`` / ``negative`` (sequences whose elements are doc ids — strings — or ``[dim]`` vectors, mixed freely) ->
        ``(vectors fp32 [P + N, dim] with zeros where an id stands, rows int64 [P + N] with -1 where a vector stands, P)``.
        Host logic only; an unknown id raises ``KeyError``."""
        from ._engine import check_examples_request

        def as_list(x):
            if x is None:
                return []
            if isinstance(x, str):
                return [x]                                   # one bare id
            if hasattr(x, "is_cuda") and x.dim() == 1:
                return [x]                                   # one bare vector (torch)
            if isinstance(x, np.ndarray) and x.ndim == 1 and x.dtype.kind in "fiu":
                return [x]                                   # one bare vector (numpy)
            return list(x)
        pos, neg = as_list(positive), as_list(negative)
        check_examples_request(len(pos), len(neg), "any", "penalty", 1.0)
        vec = np.zeros((len(pos) + len(neg), self.dim), dtype=np.float32)
        rows = np.full(len(pos) + len(neg), -1, dtype=np.int64)
        ids = [(j, e) for j, e in enumerate(pos + neg) if isinstance(e, str)]
        if ids:
            rows[[j for j, _ in ids]] = self.rows_of([e for _, e in ids])
        for j, e in enumerate(pos + neg):
            if isinstance(e, str):
                continue
            v = e.detach().cpu().numpy() if hasattr(e, "is_cuda") else np.asarray(e)
            if v.shape != (self.dim,):
                raise ValueError(f"an example is a doc id or a vector of shape ({self.dim},), got shape {v.shape}")
            vec[j] = v
        return vec, rows, len(pos)

    def search_by_examples(self, positive, negative=None, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *,
                           match: str = "any", negative_rule: str = "penalty", negative_weight: float = 1.0,
                           candidates: Optional[int] = None, filter=None, exclude_examples: bool = True) -> SearchResult:
        """Search by EXAMPLES instead of one query vector (additive; the reference has no such method; vector databases call
        it *recommend*): "more like these documents, and not like those", or "near this caption AND near this picture".
        ``positive`` (at least one) and ``negative`` are sequences of doc ids and / or ``[dim]`` vectors, at most 16 together;
        a doc id stands for its stored row, gathered on the device.

        Every document gets ONE score from its cosine similarities to the examples, each exactly what ``search`` reports for
        that pair: ``p`` = the largest (``match="any"``) or the smallest (``match="all"``: near EVERY positive) similarity to
        a positive, ``n`` = the largest similarity to a negative, and then ``p - negative_weight * max(n, 0)``
        (``negative_rule="penalty"``), or ``p`` where ``p > n`` and ``-n * n`` elsewhere (``"best_score"``: a document
        nearer to a negative than to every positive ranks behind all others, the nearest to a negative last).  The
        ``min(2k, rows offered)`` best documents by that score — ``candidates=`` up to 2048 — are blended with DEWI
        and cut to k as in ``search``.  The whole request costs one pass over the corpus per 4 examples (2 beyond 2048
        columns), not one per example.

        ``exclude_examples``: documents given as examples are not returned.  ``filter``: what ``search(filter=)`` takes for
        ONE allow-list (a mask, doc ids, rows, a ``Where``, ``dedup_filter(...)``, a prepared filter).  Returns
        ``(doc_id, adjusted score, Payload)`` tuples; ``[]`` for ``k <= 0`` or an empty filter; ``ValueError`` for k above the
        rows offered (as ``search``), for more than 16 examples, and for what the route does not serve: bf16 or l2
        indexes, ``dim % 4 != 0``, fewer than 132 or more than 4096 columns."""
        from ._engine import DeviceQueryFilters, check_examples_request, check_examples_shape
        import torch
        vec, rows, n_pos = self._example_parts(positive, negative)          # (argument errors before any build)
        check_examples_request(n_pos, len(rows) - n_pos, match, negative_rule, negative_weight)
        if isinstance(filter, DeviceQueryFilters) or is_where_list(filter) or (filter is not None and len(getattr(filter, "shape", ())) == 2):
            raise NotImplementedError("a search by examples takes one allow-list (per-query filters: not in this build)")
        self._ensure_built()
        corpus = self._corpus
        check_examples_shape(corpus.space, corpus.is_bf16, corpus.dim)
        prepared = self._prepared(filter)
        with corpus._lock, torch.cuda.device(corpus.device):
            x = torch.from_numpy(vec).to(corpus.device)
            given = np.flatnonzero(rows >= 0)
            if given.size:
                x[torch.from_numpy(given).to(corpus.device)] = corpus.emb.index_select(
                    0, torch.from_numpy(rows[given]).to(corpus.device)).float()
            exclude = None
            if exclude_examples and given.size:
                exclude = torch.from_numpy(np.unique(rows[given])).to(corpus.device)
            ids_d, sc_d = corpus.search_examples_device(x, n_pos, int(k), float(eta), float(entropy_pref), match=match,
                                                        negative_rule=negative_rule, negative_weight=float(negative_weight),
                                                        candidates=candidates, exclude=exclude, filter=prepared)
            ids_h, sc_h = ids_d.cpu().numpy(), sc_d.cpu().numpy()
        if corpus.id_offset:
            ids_h = ids_h - corpus.id_offset
        return self.results_for(ids_h, sc_h)[0]

    # ---------------------------------------------------------------- range search (additive)
    def range_search(self, query: np.ndarray, threshold: float, eta: float = 0.5, entropy_pref: float = 0.0, filter=None,
                     max_results: Optional[int] = None) -> SearchResult:
        """Every document at least as similar to ``query`` as ``threshold`` (additive; the reference has no such method):
        ``(doc_id, adjusted score, Payload)`` tuples in the order ``search`` gives its answers.

        The similarity is the one ``search`` computes (steps 1-2 of reference backends.py:414-436) and the test is
        ``sim >= threshold``; there is no cut and no k, so the result has as many rows as pass — ``[]`` when none does or the
        index is empty.  A document's adjusted score is what ``search`` would give it (the blend with ``eta`` /
        ``entropy_pref``).  ``space="l2"``: the similarity is ``-||e - q||^2``, so a radius r is ``threshold = -r * r``.
        ``filter``: one allow-list, as ``search`` takes it (a prepared filter, a bool mask, doc ids or rows).
        ``max_results``: ``ValueError`` instead of a larger result."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        lims, rows, scores, _ = self.range_search_batch(q[:1], threshold, eta, entropy_pref, filter=filter, max_results=max_results)
        m = int(lims[1])
        return self.results_for(rows[None, :m], scores[None, :m])[0]

    def range_search_batch(self, queries: np.ndarray, threshold, eta: float = 0.5, entropy_pref: float = 0.0, filter=None,
                           max_results: Optional[int] = None, sort: bool = True):
        """[B, dim] queries -> ``(lims int64 [B + 1], rows int64 [T], scores fp32 [T], sims fp32 [T])``: query j's rows are
        ``rows[lims[j]:lims[j + 1]]`` with their adjusted scores and similarities.  ``threshold``: one number or one per
        query.  ``sort=False`` leaves every query's rows ascending instead of in ``search`` order.  Per-query filters are not
        served (``NotImplementedError``).  See ``range_search``."""
        from ._engine import DeviceQueryFilters, check_thresholds
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        b = int(q.shape[0])
        thr = check_thresholds(threshold, b)
        if isinstance(filter, DeviceQueryFilters) or is_where_list(filter) or (filter is not None and len(getattr(filter, "shape", ())) == 2):
            raise NotImplementedError("range search takes one allow-list for the batch (per-query filters: not in this build)")
        if not self._doc_ids or b == 0:         # an empty index has no rows to return (and nothing to build)
            return (np.zeros(b + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32))
        self._ensure_built()
        import torch
        corpus = self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            lims, rows, sims, scores = corpus.range_search_device(
                corpus.stage_queries(q), thr, float(eta), float(entropy_pref), filter=self._prepared(filter),
                max_results=max_results, sort=sort)
            return lims.cpu().numpy(), rows.cpu().numpy(), scores.cpu().numpy(), sims.cpu().numpy()

    # ---------------------------------------------------------------- near-duplicate self-join (additive)
    def near_duplicates(self, threshold: float, max_pairs: Optional[int] = None, doc_ids: bool = False):
        """Every pair of documents at least ``threshold`` similar (additive; the reference has no such method): numpy
        ``(a int64 [P], b int64 [P], sims fp32 [P])`` — rows ``a < b``, ordered by ``(a, b)`` — or, with ``doc_ids=True``,
        ``(ids_a, ids_b, sims)`` with two lists of doc ids.

        The pair ``(a, b)`` is reported iff document ``b`` is in ``range_search`` of document ``a``'s stored embedding at
        this threshold, and ``sims`` is that similarity (``DeviceCorpus.near_duplicates_device``).  With ``batch_shadow`` the
        join runs 2048 rows per call on the matrix cores; without it, it is one dense corpus pass per 4-8 rows.  An empty
        index, or one document, has no pairs.  ``max_pairs``: ``ValueError`` instead of a larger result."""
        if len(self._doc_ids) < 2:
            a = b = np.zeros(0, np.int64)
            sims = np.zeros(0, np.float32)
        else:
            self._ensure_built()
            import torch
            corpus = self._corpus
            with corpus._lock, torch.cuda.device(corpus.device):
                a, b, sims = (t.cpu().numpy() for t in corpus.near_duplicates_device(float(threshold), max_pairs=max_pairs))
        if doc_ids:
            ids = self._doc_ids
            return [ids[i] for i in a.tolist()], [ids[i] for i in b.tolist()], sims
        return a, b, sims

    # ---------------------------------------------------------------- near-duplicate groups (additive)
    def duplicate_groups(self, threshold: float, keep: str = "dewi", doc_ids: bool = False) -> DuplicateGroups:
        """The near-duplicate groups of the index (additive; the reference has no such method): the connected components of
        the graph whose edges are the pairs ``near_duplicates(threshold)`` reports — computed on the device without ever
        holding the pairs, so a cluster of m copies costs m rows of memory, not m (m - 1) / 2 pairs, and there is no
        ``max_pairs``.  Single linkage: a chain of pairwise-similar documents is one group.

        Returns a ``DuplicateGroups``: ``labels[i]`` the smallest row of document i's group, ``sizes[i]`` the group's number of
        documents, ``representatives[i]`` the one row to keep of it — ``keep="dewi"`` the member with the highest ``dewi``
        (ties to the lower row), ``keep="first"`` the smallest row — and ``n_groups``, singletons included.  ``doc_ids=True``
        adds ``clusters``: the groups as lists of doc ids, ordered by label, members by ascending row, singletons included —
        the shape the reference's ``metrics.duplicate_rate`` / ``cluster_coverage`` take.  An empty index has no groups, one
        document is its own; neither builds anything.  (``IVFIndex`` inherits this unchanged: it is exact, the cells are not
        consulted.)"""
        from . import _native as nat
        if keep not in nat.KEEP_CODES:
            raise ValueError(f"unknown keep rule {keep!r}: one of {sorted(nat.KEEP_CODES)}")
        n = len(self._doc_ids)
        if n < 2:
            labels = np.arange(n, dtype=np.int64)
            sizes, reps, n_groups = np.ones(n, np.int64), labels.copy(), n
        else:
            self._ensure_built()
            import torch
            corpus = self._corpus
            with corpus._lock, torch.cuda.device(corpus.device):
                out, n_groups = corpus.duplicate_groups_device(float(threshold), keep=keep)
                labels, sizes, reps = (t.cpu().numpy() for t in out)
        return DuplicateGroups(labels, sizes, reps, int(n_groups), clusters_from_labels(labels, self._doc_ids) if doc_ids else None)

    def dedup_filter(self, threshold: float, keep: str = "dewi"):
        """``make_filter`` of the rows that are their group's representative in ``duplicate_groups(threshold, keep)``: a
        normal ``DeviceFilter``, so ``search(..., filter=index.dedup_filter(0.95))`` is the filtered exact search with every
        near-duplicate group collapsed to one document.  fp32 corpora, as every filter (bf16: ``NotImplementedError``).  On an
        ``IVFIndex`` a user filter already runs the parent's exact filtered search, and so does this one."""
        self._ensure_built()
        import torch
        corpus = self._corpus
        if corpus.is_bf16:
            raise NotImplementedError("filtered search serves fp32 corpora (bf16: not in this build)")
        with corpus._lock, torch.cuda.device(corpus.device):
            (_, _, reps), _ = corpus.duplicate_groups_device(float(threshold), keep=keep)
            mask = reps == torch.arange(corpus.id_offset, corpus.id_offset + corpus.n_rows, dtype=torch.int64, device=corpus.device)
        return self.make_filter(mask)

    def results_for(self, rows: np.ndarray, scores: np.ndarray) -> List[SearchResult]:
        """Row indices/scores of ``search_batch`` -> the reference's (doc_id, score, Payload) tuples."""
        ids, at_row = self._doc_ids, self._payloads.at_row
        if self._payloads._blocks:      # column blocks (possibly device-resident): one gather for the rows that are wanted
            self._payloads.ensure_rows(np.unique(np.asarray(rows)).tolist(), ids)
        return [[(ids[r], float(s), at_row(r, ids[r])) for r, s in zip(rr.tolist(), ss.tolist())]
                for rr, ss in zip(rows, scores)]

    # ---------------------------------------------------------------- persistence (reference :483-556)
    def save(self, path: Union[str, Path]) -> None:
        root = Path(path)
        root.mkdir(parents=True, exist_ok=True)
        if self._pending:
            # the file format stores rows in normalised form (the reference normalises at add());
            # here normalisation is a device kernel, so pending rows are built first
            self.build()
        emb = self._embeddings
        matrix = emb if isinstance(emb, np.ndarray) else (np.array(emb) if len(emb) else np.empty((0, self.dim), np.float32))
        with open(root / "metadata.json", "w") as fh:
            json.dump({"dim": self.dim, "space": self.space, "doc_ids": self._doc_ids, "normalize": self._normalize,
                       "is_trained": self._is_trained, "num_embeddings": int(len(matrix))}, fh)
        with open(root / "payloads.jsonl", "w") as fh:
            for doc_id in self._doc_ids:
                fh.write(json.dumps({"doc_id": doc_id, "payload": self._payloads[doc_id].to_dict()}) + "\n")
        if len(matrix) > 0:
            np.save(str(root / "embeddings.npy"), matrix)
        self._attrs_save(root)                      # attributes.npz / attributes.json, only when there are attributes

    @classmethod
    def load(cls, path: Union[str, Path], **kwargs: Any) -> "ExactIndex":
        root = Path(path)
        with open(root / "metadata.json", "r") as fh:
            meta = json.load(fh)
        inst = cls(dim=meta["dim"], space=meta["space"], **kwargs)
        inst._doc_ids = meta["doc_ids"]
        inst._normalize = meta["normalize"]
        with open(root / "payloads.jsonl", "r") as fh:
            for line in fh:
                rec = json.loads(line)
                inst._payloads[rec["doc_id"]] = Payload.from_dict(rec["payload"])
        emb_path = root / "embeddings.npy"
        if emb_path.exists() and meta.get("num_embeddings", 0) > 0:
            # rows on disk are already in stored (normalised) form — whether the reference saved them
            # before or after build() — so they are uploaded as they are
            inst._loaded_rows = np.ascontiguousarray(np.load(str(emb_path), allow_pickle=False), dtype=np.float32)
        elif inst._doc_ids:
            logger.warning("No embeddings found during load, index will need to be rebuilt")
        inst._is_trained = False  # the device copy is rebuilt lazily on the first search
        inst._attrs_load(root)
        return inst

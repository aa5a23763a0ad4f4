"""Attribute columns of an index and the predicates over them (additive; the reference has no counterpart).

Attributes are per-document columns of 4-byte values — int32, fp32, or int32 codes of a categorical column whose vocabulary
stays on the host — resident on the device next to the corpus and addressed by name.  ``AttributesMixin`` gives
``ExactIndex`` (and with it ``IVFIndex``) the methods that set, read, mutate, persist and FILTER on them: a ``dewi.where``
predicate becomes the byte mask ``dewi_filter_prepare`` / ``dewi_query_filter_prepare`` already take, made on the device by
``dewi_predicate_masks``, so every ``filter=`` accepts a ``Where``.

The host half (``encode_column``, ``write_attribute_files`` / ``read_attribute_files``) needs no device.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._native import PRED_MAX_COLUMNS
from .types import PAYLOAD_FIELDS
from .where import Where, compile_programs, is_where_list

ATTRIBUTES_FORMAT_VERSION = 1
KINDS = ("int", "float", "cat")
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def fill_value(kind: str):
    """What a row holds that was appended without attributes: int 0, float NaN, categorical -1 (missing)."""
    return {"int": 0, "float": float("nan"), "cat": -1}[kind]


def _check_int32(lo: int, hi: int, name: str) -> None:
    if lo < INT32_MIN or hi > INT32_MAX:
        raise ValueError(f"attribute {name!r}: values {lo} .. {hi} do not fit int32")


def encode_strings(values: Sequence, name: str, vocab: Optional[List[str]] = None) -> Tuple[np.ndarray, List[str]]:
    """Strings (``None``: missing) -> (int32 codes, vocabulary).  Without ``vocab`` the vocabulary is the sorted unique
    strings; with one, strings it lacks are added and the whole is sorted again (the caller re-maps the stored codes)."""
    vals = list(values)
    bad = [v for v in vals if v is not None and not isinstance(v, str)]
    if bad:
        raise ValueError(f"attribute {name!r}: a categorical column holds strings or None, got {bad[0]!r}")
    words = sorted(set(v for v in vals if v is not None) | set(vocab or ()))
    code = {s: i for i, s in enumerate(words)}
    return np.fromiter((-1 if v is None else code[v] for v in vals), dtype=np.int32, count=len(vals)), words


def encode_column(values, name: str, kind: Optional[str] = None):
    """A host array, sequence or CUDA tensor -> ``(kind, values, vocabulary)``: int32 for integers and bools (a value outside
    int32: ``ValueError``), float32 for floats (float64 is rounded once), int32 codes and the sorted vocabulary for a sequence
    of strings / ``None``.  ``kind``: what an existing column holds — numbers of the other numeric kind are converted, strings
    into a number column (or numbers into a categorical one) raise ``ValueError``."""
    if hasattr(values, "is_cuda"):
        import torch
        t = values
        if t.dtype.is_floating_point:
            got = "float"
        elif t.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            got = "int"
        else:
            raise ValueError(f"attribute {name!r}: unsupported tensor dtype {t.dtype}")
        if kind == "cat":
            raise ValueError(f"attribute {name!r} is categorical: pass strings")
        if (kind or got) == "float":
            return "float", t.to(torch.float32), None
        if got == "float":
            raise ValueError(f"attribute {name!r} holds integers, got floats")
        if t.dtype == torch.int64 and t.numel():
            _check_int32(int(t.min().item()), int(t.max().item()), name)
        return "int", t.to(torch.int32), None
    if isinstance(values, np.ndarray):
        arr = values
    else:
        seq = list(values)
        if any(v is None or isinstance(v, str) for v in seq):      # (np.asarray would turn the numbers among them into strings)
            arr = np.empty(len(seq), dtype=object)
            arr[:] = seq
        else:
            arr = np.asarray(seq)
    if arr.dtype.kind in "USO":
        if kind in ("int", "float"):
            raise ValueError(f"attribute {name!r} holds numbers, got {arr.reshape(-1)[:1].tolist()}")
        codes, vocab = encode_strings(arr.reshape(-1).tolist(), name)
        return "cat", codes.reshape(arr.shape), vocab
    if kind == "cat":
        raise ValueError(f"attribute {name!r} is categorical: pass strings")
    if arr.dtype.kind in "biu":
        if kind == "float":
            return "float", arr.astype(np.float32), None
        if arr.size:
            _check_int32(int(arr.min()), int(arr.max()), name)
        return "int", arr.astype(np.int32), None
    if arr.dtype.kind == "f":
        if kind == "int":
            raise ValueError(f"attribute {name!r} holds integers, got floats")
        with np.errstate(over="ignore"):
            return "float", arr.astype(np.float32), None
    raise ValueError(f"attribute {name!r}: unsupported dtype {arr.dtype}")


def write_attribute_files(root: Path, columns: Sequence[Tuple[str, str, np.ndarray, Optional[List[str]], bool]]) -> None:
    """``attributes.npz`` (one array per column, keyed by position) and ``attributes.json`` (names, kinds, vocabularies, which
    columns mirror a payload field) into ``root``.  ``columns``: ``(name, kind, values, vocabulary, mirror)``."""
    root = Path(root)
    np.savez(str(root / "attributes.npz"), **{f"c{i}": np.ascontiguousarray(c[2]) for i, c in enumerate(columns)})
    with open(root / "attributes.json", "w") as fh:
        json.dump({"format_version": ATTRIBUTES_FORMAT_VERSION,
                   "num_rows": int(len(columns[0][2])) if columns else 0,
                   "columns": [{"name": name, "kind": kind, "vocabulary": vocab, "mirror": bool(mirror)}
                               for name, kind, _, vocab, mirror in columns]}, fh)


def read_attribute_files(root: Path) -> Optional[List[Tuple[str, str, np.ndarray, Optional[List[str]], bool]]]:
    """What ``write_attribute_files`` wrote, or ``None`` for a folder without attributes."""
    root = Path(root)
    if not (root / "attributes.json").exists():
        return None
    with open(root / "attributes.json") as fh:
        meta = json.load(fh)
    if meta.get("format_version") != ATTRIBUTES_FORMAT_VERSION:
        raise ValueError(f"unknown attributes.json format version {meta.get('format_version')}")
    out = []
    with np.load(str(root / "attributes.npz"), allow_pickle=False) as data:
        for i, c in enumerate(meta["columns"]):
            if c["kind"] not in KINDS:
                raise ValueError(f"attributes.json: unknown kind {c['kind']!r}")
            want = np.float32 if c["kind"] == "float" else np.int32
            out.append((c["name"], c["kind"], np.ascontiguousarray(data[f"c{i}"], dtype=want), c.get("vocabulary"),
                        bool(c.get("mirror", False))))
    return out


class _Column:
    """One attribute column: ``data`` a device tensor of at least ``rows`` elements (the storage, in step with the corpus's
    capacity), the first ``rows`` of which are the column."""

    __slots__ = ("kind", "data", "rows", "vocab", "mirror")

    def __init__(self, kind: str, data, rows: int, vocab: Optional[List[str]], mirror: bool = False):
        self.kind, self.data, self.rows, self.vocab, self.mirror = kind, data, int(rows), vocab, bool(mirror)

    def view(self):
        return self.data[: self.rows]


class AttributesMixin:
    """The attribute methods of ``ExactIndex``; see the module docstring.  Expects ``_corpus``, ``_doc_ids``,
    ``_ensure_built``, ``rows_of`` and ``_payload_columns`` of the class it is mixed into."""

    def _attrs_init(self) -> None:
        self._attrs: Dict[str, _Column] = {}
        self._attrs_loaded = None           # read_attribute_files' columns of a loaded index, not yet on the device

    # ---------------------------------------------------------------- storage
    def _torch_dtype(self, kind: str):
        import torch
        return torch.float32 if kind == "float" else torch.int32

    def _attr_columns(self) -> Dict[str, _Column]:
        """The columns, on the device and as long as the index: a loaded index's columns are uploaded here, and rows that
        joined since a column was set (``add`` + ``build``, ``upsert*`` of new ids) are filled with ``fill_value``."""
        if not self._attrs and self._attrs_loaded is None:
            return self._attrs
        self._ensure_built()
        import torch
        corpus = self._corpus
        n = corpus.n_rows
        with torch.cuda.device(corpus.device):
            if self._attrs_loaded is not None:
                loaded, self._attrs_loaded = self._attrs_loaded, None
                for name, kind, values, vocab, mirror in loaded:
                    if len(values) != n:
                        raise ValueError(f"attributes.npz: column {name!r} has {len(values)} rows, the index {n}")
                    self._attrs[name] = _Column(kind, torch.from_numpy(values).to(corpus.device), n, vocab, mirror)
            cap = max(corpus.capacity, n)
            for c in self._attrs.values():
                if int(c.data.shape[0]) < cap:
                    g = torch.empty(cap, dtype=c.data.dtype, device=corpus.device)
                    g[: c.rows].copy_(c.data[: c.rows])
                    c.data = g
                if c.rows < n:
                    c.data[c.rows: n].fill_(fill_value(c.kind))
                c.rows = n
        return self._attrs

    def attribute_schema(self) -> Dict[str, Tuple[str, Optional[List[str]]]]:
        """``{name: (kind, vocabulary)}``: kind ``"int"`` / ``"float"`` / ``"cat"``; what ``Where.compile`` resolves against.
        Host logic only."""
        if self._attrs_loaded is not None:
            return {name: (kind, vocab) for name, kind, _, vocab, _ in self._attrs_loaded}
        return {name: (c.kind, c.vocab) for name, c in self._attrs.items()}

    def attribute_names(self) -> List[str]:
        return list(self.attribute_schema())

    # ---------------------------------------------------------------- set / drop / update / read
    def set_attributes(self, **columns) -> None:
        """Set attribute columns by name (additive).  Each column is a host array, a sequence or a CUDA tensor of length N:
        integers and bools are stored as int32 (a value outside int32: ``ValueError``), floats as fp32 (float64 is rounded
        once), a sequence of strings as a categorical column — int32 codes into the sorted unique values, ``None`` the code
        -1 — whose vocabulary stays on the host.  An existing name is replaced.  At most 16 columns.  Everything is checked
        before any column changes."""
        n = len(self._doc_ids)
        names = self.attribute_names()
        if len(set(names) | set(columns)) > PRED_MAX_COLUMNS:
            raise ValueError(f"an index holds at most {PRED_MAX_COLUMNS} attribute columns "
                             f"(it has {len(names)}, {len(set(columns) - set(names))} more were given)")
        made = {}
        for name, values in columns.items():
            kind, vals, vocab = encode_column(values, name)
            if tuple(vals.shape) != (n,):
                raise ValueError(f"attribute {name!r} has shape {tuple(vals.shape)}, expected ({n},)")
            made[name] = (kind, vals, vocab)
        self._ensure_built()                        # (every argument error comes before any device work)
        have = self._attr_columns()
        import torch
        corpus = self._corpus
        with torch.cuda.device(corpus.device):
            for name, (kind, vals, vocab) in made.items():
                data = torch.empty(max(corpus.capacity, n), dtype=self._torch_dtype(kind), device=corpus.device)
                data[:n].copy_(vals if hasattr(vals, "is_cuda") else torch.from_numpy(np.ascontiguousarray(vals)))
                have[name] = _Column(kind, data, n, vocab)

    def drop_attributes(self, *names: str) -> None:
        have = self._attr_columns()
        unknown = [x for x in names if x not in have]
        if unknown:
            raise ValueError(f"unknown attribute columns {unknown}")
        for x in names:
            del have[x]

    def attributes_from_payload(self, *fields: str) -> None:
        """Mirror ``Payload`` fields (``noise``, ``redundancy``, ``dewi``, ``ht_mean`` ...) as fp32 attribute columns of the
        same name, so that the DEWI signals themselves can be filtered on.  A snapshot: calling it again refreshes it, and
        ``upsert*`` refreshes the touched rows from the new payloads."""
        unknown = [f for f in fields if f not in PAYLOAD_FIELDS]
        if unknown:
            raise ValueError(f"unknown payload fields {unknown} (a Payload has {list(PAYLOAD_FIELDS)})")
        if not fields:
            return
        self._ensure_built()
        cols = self._payload_columns(tuple(fields))
        self.set_attributes(**{f: cols[f] for f in fields})
        for f in fields:
            self._attrs[f].mirror = True

    def _values_for(self, c: _Column, name: str, values, m: int):
        """``values`` for ``m`` rows of column ``c`` as a device tensor of its dtype; a categorical column may gain words."""
        import torch
        corpus = self._corpus
        if c.kind == "cat":
            vals = [values] * m if values is None or isinstance(values, str) else list(values)
            codes, words = encode_strings(vals, name, c.vocab)
            if words != c.vocab:                # new words: the vocabulary stays sorted, the stored codes move with it
                new_code = {s: i for i, s in enumerate(words)}
                remap = np.array([-1] + [new_code[s] for s in c.vocab], dtype=np.int32)
                view = c.view()
                view.copy_(torch.from_numpy(remap).to(corpus.device)[(view + 1).to(torch.int64)])
                c.vocab = words
            out = torch.from_numpy(codes)
        else:
            if np.ndim(values) == 0 and not hasattr(values, "is_cuda"):
                values = np.full(m, values)
            _, vals, _ = encode_column(values, name, c.kind)
            out = vals if hasattr(vals, "is_cuda") else torch.from_numpy(np.ascontiguousarray(vals))
        if tuple(out.shape) != (m,):
            raise ValueError(f"attribute {name!r}: {tuple(out.shape)} values for {m} documents")
        return out.to(device=corpus.device, dtype=c.data.dtype)

    def update_attributes(self, doc_ids: Sequence[str], **values) -> None:
        """Write attribute values for some documents, on the device: per column one value for all of them or one per
        document.  An unknown doc id raises ``KeyError``, an unknown column ``ValueError``; a categorical column learns new
        strings (its vocabulary stays sorted).  Filters prepared before keep the rows they listed."""
        ids = [doc_ids] if isinstance(doc_ids, str) else list(doc_ids)
        rows = self.rows_of(ids)
        have = self._attr_columns()
        unknown = [x for x in values if x not in have]
        if unknown:
            raise ValueError(f"unknown attribute columns {unknown}")
        if not ids:
            return
        import torch
        corpus = self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            at = torch.from_numpy(rows).to(corpus.device)
            staged = {name: self._values_for(have[name], name, v, len(ids)) for name, v in values.items()}
            for name, v in staged.items():
                have[name].view()[at] = v

    def attributes_of(self, doc_ids: Sequence[str]) -> Dict[str, Any]:
        """``{name: values}`` of the given documents, in their order: numpy int32 / float32 arrays, and for a categorical
        column a list of strings (``None``: missing)."""
        ids = [doc_ids] if isinstance(doc_ids, str) else list(doc_ids)
        rows = self.rows_of(ids)
        have = self._attr_columns()
        out: Dict[str, Any] = {}
        if not have:
            return out
        import torch
        corpus = self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            at = torch.from_numpy(rows).to(corpus.device)
            for name, c in have.items():
                v = c.view()[at].cpu().numpy()
                out[name] = [None if i < 0 else c.vocab[i] for i in v.tolist()] if c.kind == "cat" else v
        return out

    # ---------------------------------------------------------------- following the corpus
    def _attrs_after_remove(self, src: np.ndarray, dst: np.ndarray, n_keep: int) -> None:
        if not self._attrs:
            return
        import torch
        corpus = self._corpus
        with torch.cuda.device(corpus.device):
            s = torch.from_numpy(np.ascontiguousarray(src, dtype=np.int64)).to(corpus.device)
            d = torch.from_numpy(np.ascontiguousarray(dst, dtype=np.int64)).to(corpus.device)
            for c in self._attrs.values():
                if src.size:
                    c.data[d] = c.data[s]
                c.rows = int(n_keep)

    def _attrs_after_put(self, rows: np.ndarray, payloads, cols) -> None:
        """After an upsert: new rows are filled (``_attr_columns``), and the touched rows of mirrored payload fields take the
        new payloads' values — ``payloads`` objects or ``cols`` (one array per given field; a missing field is 0.0)."""
        if not self._attrs:
            return
        have = self._attr_columns()
        mirrored = [name for name, c in have.items() if c.mirror]
        if not mirrored:
            return
        import torch
        corpus = self._corpus
        with torch.cuda.device(corpus.device):
            at = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(corpus.device)
            for name in mirrored:
                if payloads is not None:
                    v = np.fromiter((getattr(p, name) for p in payloads), dtype=np.float64, count=len(payloads))
                else:
                    v = cols.get(name) if cols is not None else None
                    if v is None:
                        v = np.zeros(len(rows), dtype=np.float64)
                v = v if hasattr(v, "is_cuda") else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
                have[name].view()[at] = v.to(device=corpus.device, dtype=torch.float32)

    # ---------------------------------------------------------------- predicates
    def _where_masks(self, wheres: Sequence[Where], base=None):
        """Device bytes [P, N] of P predicates (``base``: a ``DeviceFilter`` of this corpus, ANDed in).  Everything the
        compiler refuses is raised before any device work."""
        from ._engine import DeviceFilter
        program = compile_programs(wheres, self)
        self._ensure_built()
        import torch
        corpus = self._corpus
        have = self._attr_columns()
        base8 = None
        if base is not None:
            if not isinstance(base, DeviceFilter):
                raise TypeError(f"base must be a prepared filter (make_filter, dedup_filter), got {type(base).__name__}")
            corpus.check_filter(base)
            base8 = base.byte_mask()
        with corpus._lock, torch.cuda.device(corpus.device):
            return corpus.predicate_masks([have[name].view() for name in program.columns], program.programs, program.sets, base8)

    def make_filter_where(self, where: Where, base=None):
        """Prepare the allow-list of the documents a predicate holds for (additive): the mask is made on the device
        (``dewi_predicate_masks``) and prepared by ``dewi_filter_prepare`` as any mask is — one synchronisation, for the
        count.  ``base``: a prepared filter of this index (``dedup_filter(0.95)`` ...) ANDed in.  A ``DeviceFilter`` like
        ``make_filter``'s: bound to the index as it stands, ``ValueError`` after a mutation."""
        if not isinstance(where, Where):
            raise TypeError(f"expected a Where (dewi.where.col), got {type(where).__name__}")
        masks = self._where_masks([where], base)
        return self._corpus.make_filter_bytes(masks[0])

    def make_query_filters_where(self, wheres: Sequence[Where], base=None):
        """One predicate per query -> ``DeviceQueryFilters`` (``dewi_query_filter_prepare``), as ``make_query_filters``."""
        if not is_where_list(wheres):
            raise TypeError("expected a non-empty sequence of Where predicates")
        import torch
        masks = self._where_masks(list(wheres), base)
        return self._corpus.make_query_filters(masks.view(torch.bool))

    def count_where(self, where: Where) -> int:
        """How many documents the predicate holds for."""
        if not isinstance(where, Where):
            raise TypeError(f"expected a Where (dewi.where.col), got {type(where).__name__}")
        import torch
        return int(self._where_masks([where])[0].sum(dtype=torch.int64).item())

    # ---------------------------------------------------------------- persistence
    def _attrs_save(self, root: Path) -> None:
        """``attributes.npz`` / ``attributes.json`` beside the index's files — only when the index has attributes."""
        if self._attrs_loaded is not None and self._corpus is None:
            columns = list(self._attrs_loaded)          # loaded and never built: write back what was read
        else:
            have = self._attr_columns()
            columns = [(name, c.kind, c.view().cpu().numpy(), c.vocab, c.mirror) for name, c in have.items()]
        if columns:
            write_attribute_files(root, columns)
        else:                                           # (a folder saved into before must not keep another index's columns)
            for name in ("attributes.npz", "attributes.json"):
                (Path(root) / name).unlink(missing_ok=True)

    def _attrs_load(self, root: Path) -> None:
        self._attrs_loaded = read_attribute_files(root)

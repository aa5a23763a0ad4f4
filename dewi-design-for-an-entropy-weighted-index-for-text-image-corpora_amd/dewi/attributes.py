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
from .facets import Facet, check_lists, facets_from_outputs, resolve_bins
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

    # ---------------------------------------------------------------- facets
    def _facet_column(self, column):
        """``(name, kind, vocabulary, device tensor [N])`` of an attribute name or of prepared group labels."""
        from ._engine import DeviceGroups
        if isinstance(column, DeviceGroups):
            self._corpus.check_groups(column)
            return "groups", "int", None, column.labels
        have = self._attr_columns()
        if not isinstance(column, str) or column not in have:
            raise ValueError(f"unknown attribute column {column!r} (the index has {list(have)})")
        c = have[column]
        return column, c.kind, c.vocab, c.view()

    def _facet_selection(self, filter, rows):
        """``(masks, lists, many)``: device bytes [P, N] or ``None``; device ``(lims, rows)`` of LOCAL rows or ``None``;
        whether the caller gets a list of results."""
        from ._engine import DeviceFilter, DeviceQueryFilters
        from .backends import filter_kwargs
        import torch
        corpus = self._corpus
        n = corpus.n_rows
        if rows is not None:
            if filter is not None:
                raise ValueError("pass filter or rows, not both")
            if not isinstance(rows, (tuple, list)) or len(rows) != 2:
                raise ValueError("rows=(lims, rows)")
            lims, ids = rows
            if hasattr(lims, "is_cuda") and hasattr(ids, "is_cuda"):
                lims, ids = lims.to(corpus.device, torch.int64), ids.to(corpus.device, torch.int64)
                if lims.dim() != 1 or int(lims.shape[0]) < 2 or ids.dim() != 1:
                    raise ValueError("rows=(lims, rows): lims [P + 1] with P >= 1 and rows [T], both 1-D")
                if ids.numel() and (int(ids.min().item()) < 0 or int(ids.max().item()) >= n):
                    raise ValueError(f"listed rows must lie in [0, {n})")
            else:
                li, ro = check_lists(lims.cpu().numpy() if hasattr(lims, "is_cuda") else lims,
                                     ids.cpu().numpy() if hasattr(ids, "is_cuda") else ids, n)
                lims, ids = torch.from_numpy(li).to(corpus.device), torch.from_numpy(ro).to(corpus.device)
            return None, (lims, ids), True
        if filter is None:
            return None, None, False
        if isinstance(filter, Where):
            return self._where_masks([filter]), None, False
        if is_where_list(filter):
            return self._where_masks(list(filter)), None, True
        if isinstance(filter, DeviceFilter):
            corpus.check_filter(filter)
            return filter.byte_mask().view(1, n), None, False
        if isinstance(filter, DeviceQueryFilters):
            corpus.check_query_filters(filter)
            return filter.masks, None, True
        if len(getattr(filter, "shape", ())) == 2:
            m = self.query_filter_masks(filter)
            m = m if hasattr(m, "is_cuda") else torch.from_numpy(np.ascontiguousarray(m))
            return m.to(corpus.device).view(torch.uint8), None, True
        m = self.filter_mask(**filter_kwargs(filter))
        m = m if hasattr(m, "is_cuda") else torch.from_numpy(np.ascontiguousarray(m))
        return m.to(corpus.device).view(torch.uint8).view(1, n), None, False

    def _facet_run(self, columns, bins, value, masks, lists, many):
        """One ``dewi_facet_run`` per column over prepared selections -> per column a ``Facet`` or a list of them."""
        import torch
        corpus = self._corpus
        vals = None
        if value is not None:
            vname, vkind, _, vals = self._facet_column(value)
            if vkind == "cat":
                raise ValueError(f"value column {vname!r} is categorical: statistics need numbers")
        out = []
        with corpus._lock, torch.cuda.device(corpus.device):
            for column, b in zip(columns, bins):
                name, kind, vocab, keys = self._facet_column(column)

                def min_max(keys=keys, groups=name == "groups"):
                    lo, hi = (int(v.item()) for v in torch.aminmax(keys))   # the one synchronisation
                    return (0, max(hi, 0)) if groups else (lo, hi)           # negative labels: ungrouped, counted as other

                fb = resolve_bins(kind, vocab, b, name, min_max)
                counts, stats = corpus.facet_device(keys, fb.key_kind, fb.n_bins, fb.key_lo, fb.edges, masks=masks, lists=lists,
                                                    values=vals)
                got = facets_from_outputs(name, fb, counts.cpu().numpy(),
                                          None if stats is None else {k: v.cpu().numpy() for k, v in stats.items()})
                out.append(got if many else got[0])
        return out

    def facet(self, column, *, filter=None, rows=None, bins=None, value=None):
        """How the selected documents are distributed over a column (additive; ``dewi_facet_run``): a ``dewi.facets.Facet``
        with one count per bin, ``other``, ``nan`` and ``total``, counted on the device in one pass over the column.

        ``column``: an attribute name, or a ``make_groups(...)`` result (the labels are the keys, negative labels go to
        ``other``).  ``bins``: see ``dewi.facets.resolve_bins`` — ``None`` (a categorical column: its vocabulary; an int
        column: ``min .. max``, one synchronisation), a tuple ``(lo, hi)`` of integers (an inclusive range) or a sequence of
        ascending edges.  ``value``: a numeric attribute whose count / min / max / sum / mean per bin become ``stats``.
        ``filter``: whatever ``search(filter=)`` takes for one allow-list — a mask, doc ids, rows, a prepared filter, a
        ``Where`` —; a list of ``Where`` or a 2-D mask gives a LIST of results, one per predicate, from one pass.
        ``rows=(lims, rows)``: host arrays or CUDA tensors, one selection per segment ``rows[lims[p]:lims[p + 1]]``, a row
        counted once per appearance; a list of results; an id outside the index raises ``ValueError``.  ``rows`` and
        ``filter`` together raise ``ValueError``.  After ``remove`` / ``upsert*`` the columns are counted as they stand; a
        stale prepared filter raises, as everywhere."""
        self._ensure_built()
        masks, lists, many = self._facet_selection(filter, rows)
        return self._facet_run([column], [bins], value, masks, lists, many)[0]

    def facets(self, columns: Sequence, *, filter=None, rows=None, bins=None, value=None) -> Dict[str, Any]:
        """``facet`` for several columns over the same selections: the predicate masks are evaluated once.  ``bins``: ``None``
        or ``{column name: bins}``.  Returns ``{column name: Facet or list}`` in the order given."""
        columns = list(columns)
        self._ensure_built()
        names = [self._facet_column(c)[0] for c in columns]
        unknown = [k for k in (bins or {}) if k not in names]
        if unknown:
            raise ValueError(f"bins given for columns {unknown} that are not counted")
        masks, lists, many = self._facet_selection(filter, rows)
        got = self._facet_run(columns, [(bins or {}).get(x) for x in names], value, masks, lists, many)
        return dict(zip(names, got))

    def facet_range(self, queries, thresholds, column, *, filter=None, value=None, bins=None):
        """One ``Facet`` per query over the documents at least ``thresholds`` similar to it (``range_search_batch``'s rows):
        the range search leaves its ``lims`` and ``rows`` on the device and ``dewi_facet_run`` counts them there — nothing of
        the size of the result crosses to the host.  ``filter``: one allow-list for the batch, as ``range_search_batch``."""
        from ._engine import DeviceQueryFilters, check_thresholds
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        thr = check_thresholds(thresholds, int(q.shape[0]))
        if isinstance(filter, DeviceQueryFilters) or is_where_list(filter) or (filter is not None and len(getattr(filter, "shape", ())) == 2):
            raise NotImplementedError("range search takes one allow-list for the batch (per-query filters: not in this build)")
        if q.shape[0] == 0:
            return []
        self._ensure_built()
        import torch
        corpus = self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            lims, rows, _, _ = corpus.range_search_device(corpus.stage_queries(q), thr, 0.0, 0.0, filter=self._prepared(filter), sort=False)
            if corpus.id_offset:
                rows = rows - corpus.id_offset
            return self._facet_run([column], [bins], value, None, (lims, rows), True)[0]

    def stratify_by_dewi(self, bins, *, filter=None, rows=None) -> Dict[Tuple[float, float], float]:
        """The reference's ``metrics.stratify_by_dewi`` over the index: ``{(lo, hi): proportion}`` of the selected documents
        whose ``dewi`` lies in each bin — ``lo <= dewi < hi``, the last bin closed at both ends —, the denominator being every
        selected document, inside a bin or not.  ``rows=(lims, rows)`` pools every segment, as the reference pools the
        rankings of all queries.  Needs the ``dewi`` attribute: call ``attributes_from_payload("dewi")`` first."""
        if bins is None or len(bins) < 2:
            raise ValueError("At least two bin boundaries required")
        if "dewi" not in self.attribute_schema():
            raise ValueError('stratify_by_dewi reads the "dewi" attribute column: call attributes_from_payload("dewi") first')
        got = self.facet("dewi", filter=filter, rows=rows, bins=list(bins))
        if isinstance(got, list):
            pooled = Facet("dewi", got[0].keys, sum(f.counts for f in got), sum(f.other for f in got), sum(f.nan for f in got))
        else:
            pooled = got
        return pooled.proportions()

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

"""Facets: how the selected documents are distributed over an attribute's values (additive; the reference's only counterpart is
``metrics.stratify_by_dewi``).  Host logic only — what a ``bins=`` argument means for a column, and the ``Facet`` result — and
importable without a device; the counting itself is ``dewi_facet_run`` (include/dewi_hip.h "FACETS"), reached through
``AttributesMixin.facet`` and ``DeviceCorpus.facet_device``.
"""
from __future__ import annotations

from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from ._native import FACET_KEY_CODES, FACET_MAX_BINS

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


class FacetBins(NamedTuple):
    """What ``dewi_facet_run`` needs to know about the bins, and what the bins are called."""
    key_kind: int
    n_bins: int
    key_lo: int
    edges: Optional[np.ndarray]     # int32 / float32 [n_bins + 1], or None for an integer range
    keys: List[Any]                 # strings (categorical), ints (a range) or (lo, hi) pairs (edges), one per bin


def _is_range(bins) -> bool:
    return isinstance(bins, tuple) and len(bins) == 2 and all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) for b in bins)


def resolve_bins(kind: str, vocab: Optional[Sequence[str]], bins, name: str = "column", min_max=None) -> FacetBins:
    """``bins=`` of ``facet`` for a column of ``kind`` (``"int"`` / ``"float"`` / ``"cat"``; group labels are ``"int"``).

    ``None``: a categorical column takes its whole vocabulary; an int column ``min .. max`` of the column — ``min_max()`` is
    called for them (one synchronisation) —; a float column needs edges.  A TUPLE of two integers ``(lo, hi)`` is the
    inclusive integer range ``lo .. hi``, one bin per value (int and categorical columns; a float column has no such
    range: two numbers are two edges).  Any other sequence of at least two
    strictly ascending numbers is taken as edges: bin i holds ``e_i <= x < e_{i+1}``, the last bin ``e_{n-1} <= x <= e_n``
    (the reference's rule in ``stratify_by_dewi``).  Edges of a float column are rounded to fp32 once and compared in fp32;
    edges of an int column are integers.  ``ValueError`` for everything else, and beyond ``FACET_MAX_BINS`` bins."""
    if kind not in ("int", "float", "cat"):
        raise ValueError(f"unknown column kind {kind!r}")
    if bins is None and kind == "cat":
        if not vocab:
            raise ValueError(f"{name}: the categorical column has no values to count")
        bins = (0, len(vocab) - 1)
    if bins is None and kind == "int":
        if min_max is None:
            raise ValueError(f"{name}: pass bins=(lo, hi) or edges")
        lo, hi = (int(v) for v in min_max())
        if hi - lo + 1 > FACET_MAX_BINS:
            raise ValueError(f"{name}: its values span {lo} .. {hi}, more than {FACET_MAX_BINS} bins: pass edges "
                             f"(bins=[e0, e1, ...]) or a narrower bins=(lo, hi)")
        bins = (lo, max(hi, lo))
    if bins is None:
        raise ValueError(f"{name}: a float column needs edges (bins=[e0, e1, ...])")
    if _is_range(bins) and kind != "float":
        lo, hi = int(bins[0]), int(bins[1])
        if hi < lo:
            raise ValueError(f"{name}: empty range bins=({lo}, {hi})")
        if lo < INT32_MIN or hi > INT32_MAX:
            raise ValueError(f"{name}: bins=({lo}, {hi}) does not fit int32")
        if hi - lo + 1 > FACET_MAX_BINS:
            raise ValueError(f"{name}: bins=({lo}, {hi}) is more than {FACET_MAX_BINS} bins: pass edges (bins=[e0, e1, ...])")
        if kind == "cat":
            words = list(vocab or ())
            keys = [words[c] if 0 <= c < len(words) else None for c in range(lo, hi + 1)]
        else:
            keys = list(range(lo, hi + 1))
        return FacetBins(FACET_KEY_CODES["i32_range"], hi - lo + 1, lo, None, keys)
    if kind == "cat":
        raise ValueError(f"{name}: a categorical column is counted per value: bins=None or a range of codes")
    if isinstance(bins, (str, bytes)) or not hasattr(bins, "__len__"):
        raise ValueError(f"{name}: bins must be None, (lo, hi) or a sequence of ascending edges, got {bins!r}")
    given = list(np.asarray(bins).reshape(-1).tolist()) if hasattr(bins, "dtype") else list(bins)
    if len(given) < 2:
        raise ValueError(f"{name}: at least two edges are required, got {len(given)}")
    if len(given) - 1 > FACET_MAX_BINS:
        raise ValueError(f"{name}: {len(given) - 1} bins exceed {FACET_MAX_BINS}")
    if any(isinstance(b, (str, bytes, bool)) or b is None for b in given):
        raise ValueError(f"{name}: edges must be numbers, got {given[:3]}")
    if kind == "int":
        if any(float(b) != int(b) for b in given):
            raise ValueError(f"{name}: the edges of an int column are integers, got {given[:3]}")
        if min(given) < INT32_MIN or max(given) > INT32_MAX:
            raise ValueError(f"{name}: edges outside int32")
        edges = np.asarray([int(b) for b in given], dtype=np.int32)
        key_kind = FACET_KEY_CODES["i32_edges"]
        given = [int(b) for b in given]
    else:
        with np.errstate(over="ignore"):
            edges = np.asarray(given, dtype=np.float64).astype(np.float32)
        if np.isnan(edges).any():
            raise ValueError(f"{name}: an edge is NaN")
        key_kind = FACET_KEY_CODES["f32_edges"]
        given = [float(b) for b in given]
    if not bool(np.all(edges[1:] > edges[:-1])):
        raise ValueError(f"{name}: edges must be strictly ascending" + (" (in fp32)" if kind == "float" else ""))
    return FacetBins(key_kind, len(edges) - 1, 0, edges, [(given[i], given[i + 1]) for i in range(len(given) - 1)])


class Facet:
    """The distribution of one selection of documents over a column's bins.

    ``keys``: one per bin — strings (categorical; ``None``: a code without a word), ints (an integer range) or ``(lo, hi)``
    pairs (edges).  ``counts`` int64 per bin; ``other``: selected rows outside every bin (a missing category, a value outside
    the range or the edges); ``nan``: selected rows whose key is NaN; ``total``: every selected row.  ``stats``: ``None``, or
    a dict of per-bin arrays over the value column — ``count`` (values that are not NaN), ``min``, ``max``, ``sum``, ``mean``
    (NaN for a bin without values)."""

    __slots__ = ("column", "keys", "counts", "other", "nan", "stats")

    def __init__(self, column: str, keys: Sequence[Any], counts, other: int, nan: int, stats: Optional[Dict[str, np.ndarray]] = None):
        self.column = column
        self.keys = list(keys)
        self.counts = np.asarray(counts, dtype=np.int64)
        if self.counts.shape != (len(self.keys),):
            raise ValueError(f"{len(self.keys)} keys for counts of shape {self.counts.shape}")
        self.other, self.nan, self.stats = int(other), int(nan), stats

    @property
    def total(self) -> int:
        return int(self.counts.sum()) + self.other + self.nan

    def top(self, n: Optional[int] = None) -> List[Tuple[Any, int]]:
        """``(key, count)`` pairs by count descending, ties by key ascending (the bins' own order); the first ``n``."""
        order = sorted(range(len(self.keys)), key=lambda i: (-int(self.counts[i]), i))
        return [(self.keys[i], int(self.counts[i])) for i in (order if n is None else order[: max(int(n), 0)])]

    def proportions(self) -> Dict[Any, float]:
        """``{key: count / total}``: the denominator is every selected row, inside a bin or not (the reference's rule in
        ``stratify_by_dewi``); all 0.0 for an empty selection."""
        t = self.total
        return {k: (int(c) / t if t > 0 else 0.0) for k, c in zip(self.keys, self.counts.tolist())}

    def as_dict(self) -> Dict[str, Any]:
        out = {"column": self.column, "keys": list(self.keys), "counts": self.counts.tolist(), "other": self.other, "nan": self.nan,
               "total": self.total}
        if self.stats is not None:
            out["stats"] = {k: v.tolist() for k, v in self.stats.items()}
        return out

    def __repr__(self) -> str:
        return f"Facet({self.column!r}: {len(self.keys)} bins, {self.total} rows, {self.other} other, {self.nan} nan)"


def facets_from_outputs(column: str, bins: FacetBins, counts: np.ndarray, stats: Optional[Dict[str, np.ndarray]] = None) -> List[Facet]:
    """Host arrays ``[P, n_bins + 2]`` of ``dewi_facet_run`` -> P ``Facet``s (``stats``: ``vcount`` / ``vmin`` / ``vmax`` / ``vsum``)."""
    n = bins.n_bins
    out = []
    for p in range(counts.shape[0]):
        st = None
        if stats is not None:
            cnt = stats["vcount"][p, :n].copy()
            vsum = stats["vsum"][p, :n].copy()
            with np.errstate(invalid="ignore", divide="ignore"):
                mean = np.where(cnt > 0, vsum.astype(np.float64) / np.maximum(cnt, 1), np.nan)
            st = {"count": cnt, "min": stats["vmin"][p, :n].copy(), "max": stats["vmax"][p, :n].copy(), "sum": vsum, "mean": mean}
        out.append(Facet(column, bins.keys, counts[p, :n], counts[p, n], counts[p, n + 1], st))
    return out


def check_lists(lims, rows, n_rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """A user's HOST ``rows=(lims, rows)``: int64 arrays, ``lims`` non-decreasing from 0 to ``len(rows)``, every id in
    ``[0, n_rows)`` (``ValueError`` otherwise)."""
    li, ro = np.asarray(lims), np.asarray(rows)
    if li.ndim != 1 or li.size < 2 or ro.ndim != 1:
        raise ValueError("rows=(lims, rows): lims [P + 1] with P >= 1 and rows [T], both 1-D")
    if (li.size and not np.issubdtype(li.dtype, np.integer)) or (ro.size and not np.issubdtype(ro.dtype, np.integer)):
        raise ValueError("rows=(lims, rows) must be integers")
    li, ro = li.astype(np.int64), ro.astype(np.int64)
    if int(li[0]) != 0 or int(li[-1]) != ro.size or bool(np.any(np.diff(li) < 0)):
        raise ValueError(f"lims must ascend from 0 to len(rows) = {ro.size}")
    if ro.size and (int(ro.min()) < 0 or int(ro.max()) >= n_rows):
        raise ValueError(f"listed rows must lie in [0, {n_rows})")
    return li, ro

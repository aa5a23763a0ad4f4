"""Device-resident corpus + thin wrappers over the C ABI.

``DeviceCorpus`` owns what the search path needs in HBM — the N x d embedding matrix
(row-major, already normalised for cosine) and the two fp32 payload columns the re-rank
reads — and turns a query batch into (row ids, adjusted scores) with exactly two kernel
launches (scan, select/re-rank).  PyTorch is used only for device memory, streams and
host<->device copies.
"""
from __future__ import annotations

import ctypes
import itertools
import threading
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import _native as nat

ArrayLike = Union[np.ndarray, "torch.Tensor"]  # noqa: F821


def _torch():
    import torch
    return torch


_corpus_ids = itertools.count(1)


def check_thresholds(thresholds, n_queries: int) -> np.ndarray:
    """A scalar or [B] thresholds -> fp32 [B] host array (``ValueError`` for any other shape).  Host logic only."""
    t = np.asarray(thresholds, dtype=np.float32)
    if t.ndim == 0 or t.shape == (1,):
        return np.full(n_queries, t.reshape(-1)[0], dtype=np.float32)
    if t.shape != (n_queries,):
        raise ValueError(f"thresholds must be a scalar or have shape ({n_queries},), got {t.shape}")
    return np.ascontiguousarray(t)


# ---- what every search entry point shares (host logic only: plain functions of shapes and values) ----------------------
def check_search_args(q_shape, dim: int, k, candidates: Optional[int], similarity: str) -> Tuple[int, int]:
    """The argument check of the three ``DeviceCorpus`` search paths and ``IVFIndex.search_device``, in one order: query
    width, ``similarity``, "a transform needs ``candidates``" -> ``(batch, k)``.  ``k <= 0`` is the caller's next question."""
    if q_shape[1] != dim:
        raise ValueError(f"Expected query shape ({dim},), got {tuple(q_shape[1:])}")
    if similarity not in nat.SIM_CODES:
        raise ValueError(f"unknown similarity {similarity!r}")
    if candidates is None and similarity != "ip":
        raise ValueError("similarity transforms belong to the ANN re-rank rule: pass candidates=k as well")
    return int(q_shape[0]), int(k)


def cut_size(k: int, candidates: Optional[int], n: Optional[int] = None) -> int:
    """The similarity cut that is re-ranked: the reference's ``2k`` (backends.py:439) or ``candidates``, at most the ``n``
    rows there are to choose from (``None``: the caller has made sure of that already), never below 1."""
    c = 2 * int(k) if candidates is None else int(candidates)
    if n is not None:
        c = min(c, int(n))
    return max(c, 1)


def check_int8_shape(space: str, is_bf16: bool, dim: int) -> None:
    """What the int8 route serves: cosine, an fp32 main matrix, ``dim % 16 == 0`` up to 4096 columns — anything else is a
    ``ValueError``.  Host logic only."""
    if space != "cosine":
        raise ValueError(f"the int8 shadow serves cosine corpora, not space={space!r}")
    if is_bf16:
        raise ValueError("the int8 shadow is made from an fp32 main matrix (this corpus is bf16)")
    if int(dim) % 16 != 0 or not 16 <= int(dim) <= nat.I8_MAX_DIM:
        raise ValueError(f"the int8 shadow takes dim % 16 == 0 from 16 to {nat.I8_MAX_DIM} columns, got dim = {dim}")


#: largest candidate cut of a search by examples (what one workgroup of the select sorts: 2048 records)
EXAMPLES_MAX_CANDIDATES = 2048


def check_examples_shape(space: str, is_bf16: bool, dim: int) -> None:
    """What a search by examples serves: cosine, an fp32 corpus, ``dim % 4 == 0`` from 132 to 4096 columns — anything else
    is a ``ValueError``.  Host logic only."""
    if space != "cosine":
        raise ValueError(f"a search by examples serves cosine corpora, not space={space!r}")
    if is_bf16:
        raise ValueError("a search by examples serves fp32 corpora (this corpus is bf16)")
    if int(dim) % 4 != 0 or not 132 <= int(dim) <= 4096:
        raise ValueError(f"a search by examples takes dim % 4 == 0 from 132 to 4096 columns, got dim = {dim}")


def check_examples_request(n_positive: int, n_negative: int, match: str, negative_rule: str, negative_weight) -> Tuple[int, int]:
    """A request's counts and rules: at least one positive, at most ``EXAMPLES_MAX`` = 16 examples, ``match`` "any" / "all",
    ``negative_rule`` "penalty" / "best_score", a weight that is finite in fp32 — ``ValueError`` otherwise.  Host logic only."""
    if n_positive < 1:
        raise ValueError("a search by examples needs at least one positive example")
    if n_negative < 0:
        raise ValueError(f"n_negative must be >= 0, got {n_negative}")
    if n_positive + n_negative > nat.EXAMPLES_MAX:
        raise ValueError(f"a search by examples takes at most {nat.EXAMPLES_MAX} examples, got {n_positive + n_negative}")
    if match not in nat.EXAMPLES_MATCH_CODES:
        raise ValueError(f"unknown match {match!r} (one of {sorted(nat.EXAMPLES_MATCH_CODES)})")
    if negative_rule not in nat.EXAMPLES_RULE_CODES:
        raise ValueError(f"unknown negative_rule {negative_rule!r} (one of {sorted(nat.EXAMPLES_RULE_CODES)})")
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(negative_weight)):
            raise ValueError(f"negative_weight must be finite in fp32, got {negative_weight!r}")
    return n_positive, n_negative


def approx_cut(k: int, candidates: Optional[int], n: int) -> int:
    """The cut of an approximate search: the project's one rule (``cut_size``: ``min(2k, n)``, or ``candidates``), which the
    int8 route serves up to ``I8_MAX_CANDIDATES``; ``k`` must fit into it.  ``ValueError`` otherwise.  Host logic only."""
    if candidates is not None and int(candidates) > nat.I8_MAX_CANDIDATES:
        raise ValueError(f"the int8 route re-ranks at most {nat.I8_MAX_CANDIDATES} candidates, got candidates = {int(candidates)}")
    c = cut_size(k, candidates, n)
    if c > nat.I8_MAX_CANDIDATES:
        raise ValueError(f"the int8 route re-ranks at most {nat.I8_MAX_CANDIDATES} candidates, k = {int(k)} asks for {c}")
    if int(k) > c:
        raise ValueError(f"k = {int(k)} exceeds the cut of {c} candidates")
    return c


def check_binary_shape(space: str, is_bf16: bool, dim: int) -> None:
    """What the binary route serves: cosine, an fp32 main matrix, ``dim % 128 == 0`` from 128 to 4096 columns (rows of whole
    128-bit units) — anything else is a ``ValueError``.  Host logic only."""
    if space != "cosine":
        raise ValueError(f"the binary shadow serves cosine corpora, not space={space!r}")
    if is_bf16:
        raise ValueError("the binary shadow is made from an fp32 main matrix (this corpus is bf16)")
    if int(dim) % nat.B1_MIN_DIM != 0 or not nat.B1_MIN_DIM <= int(dim) <= nat.I8_MAX_DIM:
        raise ValueError(f"the binary shadow takes dim % {nat.B1_MIN_DIM} == 0 from {nat.B1_MIN_DIM} to {nat.I8_MAX_DIM} columns, "
                         f"got dim = {dim}")


def binary_cut(k: int, candidates: Optional[int], n: int) -> int:
    """The cut of a binary search: ``min(n, 1024, max(128, 16 k))`` by default — a Hamming score is far coarser than an int8
    one, so the cut is wider than the project's ``2k`` (recall per cut: DESIGN.md 4.1aa) —, or ``candidates`` (at most
    ``I8_MAX_CANDIDATES`` = 1024, the re-scoring kernel's limit; at most the ``n`` rows there are).  ``k`` must fit into it.
    ``ValueError`` otherwise.  Host logic only."""
    if candidates is None:
        c = min(int(n), nat.I8_MAX_CANDIDATES, max(128, 16 * int(k)))
    else:
        if int(candidates) > nat.I8_MAX_CANDIDATES:
            raise ValueError(f"the binary route re-ranks at most {nat.I8_MAX_CANDIDATES} candidates, got candidates = {int(candidates)}")
        c = min(int(candidates), int(n))
    c = max(c, 1)
    if int(k) > c:
        raise ValueError(f"k = {int(k)} exceeds the cut of {c} candidates")
    return c


def library_size(size_fn, *args) -> int:
    """``size_fn(*args)`` in bytes.  A size function of the library answers 0 for a shape it refuses: ``NativeLibraryError``
    with its last error."""
    need = int(size_fn(*args))
    if need == 0:
        raise nat.NativeLibraryError(f"{getattr(size_fn, '__name__', size_fn)} returned 0: " + nat.last_error())
    return need


def default_outputs(b: int, k: int, device, out_ids=None, out_scores=None):
    """The caller's output tensors, or fresh ``[B, k]`` ones (ids int64, scores fp32) where it gave none."""
    torch = _torch()
    if out_ids is None:
        out_ids = torch.empty((b, k), dtype=torch.int64, device=device)
    if out_scores is None:
        out_scores = torch.empty((b, k), dtype=torch.float32, device=device)
    return out_ids, out_scores


def empty_result(b: int, device):
    """The ``[B, 0]`` answer of a search with nothing to return (k <= 0, an empty filter)."""
    return default_outputs(b, 0, device)


# The library's launch-shape overrides are thread-local, and the workspace sizes depend on them: ``tuning()`` stamps the
# calling thread with a fresh process-wide number, a thread that never called it keeps 0 (the defaults).  Two threads with
# the same number therefore have the same tuning, whatever their idents.
_tuning_epochs = itertools.count(1)
_thread_tuning = threading.local()


def _order_key(x):
    """fp32 tensor -> int64 keys in the order of the kernels' ``ord_f32``: larger float, larger key; -0 == +0; NaN on top."""
    torch = _torch()
    u = (x + 0.0).view(torch.int32).to(torch.int64)
    k = torch.where(u >= 0, u, -(u & 0x7FFFFFFF))
    return torch.where(torch.isnan(x), torch.full_like(k, 1 << 31), k)


#: an append beyond the capacity grows the storage to ``max(needed, capacity + capacity // CAPACITY_GROWTH_DIVISOR)`` rows
CAPACITY_GROWTH_DIVISOR = 4


def plan_remove(n_rows: int, rows) -> Tuple[np.ndarray, np.ndarray, int]:
    """The moves of a removal: ``(src int64 [p], dst int64 [p], n_keep)``.  Host logic only (NumPy).

    Rows are not shifted down; the tail fills the holes.  With ``n_keep = n_rows - len(rows)``: the holes are the deleted
    rows below ``n_keep``, ascending; the movers are the surviving rows of ``[n_keep, n_rows)``, ascending; there are as
    many of one as of the other, mover i goes to hole i (``src[i] -> dst[i]``) and the corpus is cut to ``n_keep`` rows.
    Sources lie at or above ``n_keep`` and destinations below it, so the move is in place and touches at most ``len(rows)``
    rows.  ``ValueError``: rows that are not integers, out of range or repeated, or a removal of every row."""
    n = int(n_rows)
    r = np.asarray(rows).reshape(-1)
    if r.size and not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"rows to remove must be integers, got {r.dtype}")
    r = np.sort(r.astype(np.int64))
    m = int(r.size)
    if m and (int(r[0]) < 0 or int(r[-1]) >= n):
        raise ValueError(f"rows to remove must lie in [0, {n})")
    if m > 1 and bool((np.diff(r) == 0).any()):
        raise ValueError("rows to remove must be distinct")
    if m >= n and n > 0:
        raise ValueError(f"cannot remove every row ({m} of {n}): an index keeps at least one document")
    n_keep = n - m
    first_tail = int(np.searchsorted(r, n_keep))
    dst = r[:first_tail].copy()
    survives = np.ones(m, dtype=bool)
    survives[r[first_tail:] - n_keep] = False
    src = n_keep + np.flatnonzero(survives).astype(np.int64)
    return src, dst, n_keep


FILTER_HEADER_WORDS = 16       # kFilterHeaderWords (csrc/launch.hpp): a prepared filter lists its rows from this u32 word on


class DeviceFilter:
    """A prepared allow-list of corpus rows (``DeviceCorpus.make_filter``): the device buffer the filtered row kernels walk
    (``dewi_filter_prepare``: the allowed rows, sorted, grouped by the residue of their offset inside a 16-byte unit), the
    number of allowed rows and the identity of the corpus it was prepared for.  Prepare once, search many times; a filter
    used with another corpus — an index rebuilt since — raises ``ValueError`` instead of answering from stale rows."""

    __slots__ = ("buf", "n_allowed", "corpus_id", "n_rows", "_mask")

    def __init__(self, buf, n_allowed: int, corpus_id: int, n_rows: int):
        self.buf = buf
        self.n_allowed = int(n_allowed)
        self.corpus_id = int(corpus_id)
        self.n_rows = int(n_rows)
        self._mask = None

    def byte_mask(self):
        """The allow-list as device bytes [n_rows] (1 = allowed), what ``dewi_ivf_probe_prepare_filtered`` gathers from: built
        from the listed rows at the first call (zeros, ones scattered at the rows from word 16 of the buffer) and kept."""
        if self._mask is None:
            torch = _torch()
            with torch.cuda.device(self.buf.device):
                rows = self.buf.view(torch.int32)[FILTER_HEADER_WORDS: FILTER_HEADER_WORDS + self.n_allowed]
                mask = torch.zeros(self.n_rows, dtype=torch.uint8, device=self.buf.device)
                mask[rows.to(torch.int64) & 0xFFFFFFFF] = 1
            self._mask = mask
        return self._mask

    def __len__(self) -> int:
        return self.n_allowed

    def __repr__(self) -> str:
        return f"DeviceFilter({self.n_allowed} of {self.n_rows} rows)"


class DeviceQueryFilters:
    """Prepared per-query allow-lists (``DeviceCorpus.make_query_filters``): query j of a batch of ``n_queries`` searches
    only the rows of its own list F_j.  Holds the device buffer ``dewi_query_filter_prepare`` made (the union U of the lists,
    prepared like one filter, plus one word of query bits per 32 queries for every row of U), the device masks, |U|
    (``n_union``) and |F_j| (``n_allowed``, int64 [n_queries]).  Stale-checked like ``DeviceFilter``: a set used with
    another corpus raises ``ValueError``."""

    __slots__ = ("buf", "masks", "n_allowed", "n_union", "corpus_id", "n_rows", "_singles", "_subsets")

    def __init__(self, buf, masks, n_allowed, n_union: int, corpus_id: int, n_rows: int):
        self.buf = buf
        self.masks = masks                      # device uint8 [n_queries, n_rows]: lists of queries searched on their own
        self.n_allowed = np.asarray(n_allowed, dtype=np.int64)
        self.n_union = int(n_union)
        self.corpus_id = int(corpus_id)
        self.n_rows = int(n_rows)
        self._singles: Dict[int, DeviceFilter] = {}
        self._subsets: Dict[Tuple[int, ...], "DeviceQueryFilters"] = {}

    @property
    def n_queries(self) -> int:
        return int(self.n_allowed.shape[0])

    def __len__(self) -> int:
        return self.n_queries

    def __repr__(self) -> str:
        return (f"DeviceQueryFilters({self.n_queries} queries, {int(self.n_allowed.min())}-{int(self.n_allowed.max())} "
                f"of {self.n_rows} rows each, union {self.n_union})")


class DeviceGroups:
    """Prepared group labels of a corpus (``DeviceCorpus.make_groups``) for ``search_collapsed*``: ``labels`` is the device
    int32 tensor [N] ``dewi_collapse_rerank`` gathers from (negative: ungrouped, a group of its own), ``n_groups`` the number of
    groups (every ungrouped row counting as one).  Stale-checked like ``DeviceFilter``: labels used with another corpus — a
    rebuild, ``remove``, ``upsert*`` — raise ``ValueError`` instead of folding the wrong rows."""

    __slots__ = ("labels", "n_groups", "corpus_id", "n_rows")

    def __init__(self, labels, n_groups: int, corpus_id: int, n_rows: int):
        self.labels = labels
        self.n_groups = int(n_groups)
        self.corpus_id = int(corpus_id)
        self.n_rows = int(n_rows)

    def __len__(self) -> int:
        return self.n_groups

    def __repr__(self) -> str:
        return f"DeviceGroups({self.n_groups} groups over {self.n_rows} rows)"


def group_labels(groups, n_rows: int, row_of=None) -> Tuple[np.ndarray, int]:
    """What ``make_groups`` takes -> ``(labels int32 [n_rows], n_groups)``.  Host logic only (NumPy).

    ``groups``: an object with a ``labels`` array (``DuplicateGroups``); an integer array [N] in row order (negative:
    ungrouped); a sequence of N hashables, factorised in order of first appearance (``None``: ungrouped); or a mapping
    ``doc_id -> hashable`` with ``row_of`` the index's ``doc_id -> row`` (documents not named are ungrouped, ``None`` values too;
    an unknown doc id raises ``KeyError``).  ``ValueError``: a wrong length, integer labels outside int32.  ``n_groups``
    counts every distinct non-negative label and every ungrouped row."""
    n = int(n_rows)
    if hasattr(groups, "labels") and not isinstance(groups, dict):
        groups = groups.labels
    if hasattr(groups, "is_cuda"):
        groups = groups.detach().cpu().numpy()

    def factorise(pairs) -> np.ndarray:
        out = np.full(n, -1, dtype=np.int64)
        codes: Dict[object, int] = {}
        for row, value in pairs:
            if value is not None:
                out[row] = codes.setdefault(value, len(codes))
        return out

    if hasattr(groups, "keys") and hasattr(groups, "__getitem__") and not isinstance(groups, np.ndarray):
        if row_of is None:
            raise ValueError("a doc_id -> group mapping needs an index (ExactIndex.make_groups)")
        missing = [d for d in groups.keys() if d not in row_of]
        if missing:
            raise KeyError(f"unknown doc ids: {sorted(missing, key=str)[:5]}")
        lab = factorise((row_of[d], groups[d]) for d in groups.keys())
    else:
        arr = groups if isinstance(groups, np.ndarray) else None
        if arr is None:
            items = list(groups)
            if len(items) != n:
                raise ValueError(f"group labels must have length {n}, got {len(items)}")
            if items and all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) for x in items):
                arr = np.asarray(items, dtype=np.int64)
            else:
                lab = factorise(enumerate(items))
        if arr is not None:
            if arr.shape != (n,):
                raise ValueError(f"group labels must have shape ({n},), got {tuple(arr.shape)}")
            if not np.issubdtype(arr.dtype, np.integer):
                return group_labels(arr.tolist(), n, row_of)        # an object / string array: a sequence of hashables
            lab = arr.astype(np.int64) if arr.dtype != np.uint64 else arr
            if n and (int(lab.max()) > 0x7FFFFFFF or int(lab.min()) < -0x80000000):
                raise ValueError("group labels must fit int32")
    lab = np.asarray(lab)
    grouped = lab[lab >= 0]
    n_groups = int(np.unique(grouped).size) + int(lab.size - grouped.size)
    return np.ascontiguousarray(lab.astype(np.int32)), n_groups


def dense_group_labels(groups, n_rows: int, row_of=None) -> Tuple[np.ndarray, Dict[object, int]]:
    """What ``make_groups`` takes (or a ``DeviceGroups``) -> ``(labels int32 [n_rows], {group value: dense label})`` for the
    group quotas of ``select_subset_grouped``: the labels are DENSE, ``0 .. G-1``, ungrouped rows -1 — ``DuplicateGroups``
    labels and user integers can be sparse up to 2^31, and ``DeviceGroups.n_groups`` counts ungrouped rows, neither of which
    sizes a count per group.  Integer labels are numbered in ascending order of their value, hashables in order of first
    appearance by row; the map is keyed by the caller's own values (Python ints for integer labels).  Host logic only (NumPy);
    the errors are ``group_labels``'."""
    n = int(n_rows)
    if hasattr(groups, "labels") and not isinstance(groups, dict):
        groups = groups.labels
    if hasattr(groups, "is_cuda"):
        groups = groups.detach().cpu().numpy()
    values = arr = None
    if hasattr(groups, "keys") and hasattr(groups, "__getitem__") and not isinstance(groups, np.ndarray):
        group_labels(groups, n, row_of)                      # its checks: an index, unknown doc ids
        values = [None] * n
        for d in groups.keys():
            values[row_of[d]] = groups[d]
    elif isinstance(groups, np.ndarray) and np.issubdtype(groups.dtype, np.integer):
        arr = groups
    else:
        values = groups.tolist() if isinstance(groups, np.ndarray) else list(groups)
        if values and all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) for x in values):
            arr, values = np.asarray(values, dtype=np.int64), None
    if arr is not None:
        lab = group_labels(arr, n)[0].astype(np.int64)       # its checks: the shape, int32
        uniq = np.unique(lab[lab >= 0])
        dense = np.where(lab >= 0, np.searchsorted(uniq, lab), -1).astype(np.int32)
        return np.ascontiguousarray(dense), {int(v): i for i, v in enumerate(uniq.tolist())}
    if len(values) != n:
        raise ValueError(f"group labels must have length {n}, got {len(values)}")
    dense = np.full(n, -1, dtype=np.int32)
    codes: Dict[object, int] = {}
    for row, value in enumerate(values):
        if value is not None:
            dense[row] = codes.setdefault(value, len(codes))
    return dense, codes


def grouped_quotas(codes: Dict[object, int], per_group: int, quotas=None, seed_labels=()) -> Optional[np.ndarray]:
    """The quota array of ``select_subset_grouped`` (int32 [G]) or ``None`` when ``per_group`` serves every group: ``quotas``
    maps a group value to its quota (an unknown value: ``KeyError``) and overrides ``per_group``; every dense label in
    ``seed_labels`` — the groups of the seeds that count — lowers its group's quota by one.  Host logic only."""
    if int(per_group) <= 0:
        raise ValueError(f"per_group must be at least 1, got {per_group}")
    seed_labels = [int(g) for g in seed_labels if int(g) >= 0]
    if not quotas and not seed_labels:
        return None
    q = np.full(len(codes), int(per_group), dtype=np.int64)
    for value, quota in (quotas or {}).items():
        if value not in codes:
            raise KeyError(f"quotas names an unknown group: {value!r}")
        q[codes[value]] = int(quota)
    np.subtract.at(q, seed_labels, 1)
    return np.clip(q, -0x80000000, 0x7FFFFFFF).astype(np.int32)


def collapse_pool(k: int, candidates: Optional[int], n: int, approx: bool = False) -> int:
    """The pool of a collapsed search: ``candidates`` (default ``4k``), at most the ``n`` rows there are to choose from and at
    most what one re-rank takes (``COLLAPSE_MAX_CANDIDATES``; ``I8_MAX_CANDIDATES`` on the int8 route).  Host logic only."""
    cap = min(nat.COLLAPSE_MAX_CANDIDATES, nat.I8_MAX_CANDIDATES) if approx else nat.COLLAPSE_MAX_CANDIDATES
    return min(cut_size(k, 4 * int(k) if candidates is None else int(candidates), n), cap)


#: smallest range batch that goes through the bf16 shadow (DeviceCorpus.range_shadow_min_batch): the smallest MEASURED batch at
#: which the shadow route wins at 1 M x 768 — 8 queries 0.40 ms against 1.27 ms dense (profiles/r08/range_shadow/); smaller
#: batches have not been measured
RANGE_SHADOW_MIN_BATCH = 8


class _RangeBudget:
    """``max_results`` of one range call across its chunks and routes: the rows so far, and the queries they belong to."""

    def __init__(self, max_results, n_queries: int):
        self.max_results = None if max_results is None else int(max_results)
        self.n_queries = int(n_queries)
        self.total = 0
        self.done = 0

    def add(self, rows: int, queries: int) -> None:
        self.total += int(rows)
        self.done += int(queries)
        if self.max_results is not None and self.total > self.max_results:
            raise ValueError(f"range search found more than max_results = {self.max_results} rows "
                             f"({self.total} after {self.done} of {self.n_queries} queries): raise the threshold or max_results")


#: When int8 batches take the matrix-core pass by default (``batch_pass=None``): corpora of at least this many rows, or —
#: whatever the corpus — batches of at least ``I8_BATCH_AUTO_MIN_BATCH`` queries.  The C entry point itself takes 4096 rows and
#: 2 queries.  Measured at 768 columns (profiles/r20/int8_batch/crossover_rows.txt): at 4096, 16 384 and 65 536
#: rows the pass's seven launches lost to the row passes at 2 queries (0.08 against 0.06 ms) and tied at 4, and won every round
#: from 8 queries on; at 262 144 rows and 1 M it won every round from 2 queries on.
I8_BATCH_AUTO_MIN_ROWS = 262144
I8_BATCH_AUTO_MIN_BATCH = 8


class DeviceCorpus:
    """Embedding block + payload columns of one doc-id shard, resident on one GPU."""

    def __init__(self, emb, dewi32, ent32, space: str = "cosine", id_offset: int = 0):
        torch = _torch()
        if space not in nat.SPACE_CODES:
            raise ValueError(f"unknown space {space!r}")
        assert emb.is_cuda and emb.dim() == 2 and emb.is_contiguous()
        assert emb.dtype in (torch.float32, torch.bfloat16)
        self.emb = emb
        self.dewi32 = dewi32.contiguous()
        self.ent32 = ent32.contiguous()
        assert self.dewi32.dtype == torch.float32 and self.ent32.dtype == torch.float32
        assert self.dewi32.numel() == emb.shape[0] == self.ent32.numel()
        self.space = space
        self.id_offset = int(id_offset)
        self.device = emb.device
        self.corpus_id = next(_corpus_ids)      # what a DeviceFilter is checked against
        self._lib = nat.load_library()
        self._ws: Dict[tuple, tuple] = {}       # key -> (workspace, tuning epoch it was sized under): _cached_workspace
        self._q_pinned = None
        self._q_dev = None
        self.shadow = None            # bf16 copy of an fp32 matrix (enable_bf16_shadow): pre-selection over half the bytes
        self.shadow_min_batch = 2     # smallest batch that goes through the shadow (enable_bf16_shadow(single_query=True): 1)
        self.range_shadow_min_batch = RANGE_SHADOW_MIN_BATCH   # smallest range batch that goes through the shadow
        self.range_shadow_seg_cap = 32                         # records per survivor segment of its pass (dewi_hip.h seg_cap)
        self._io: Dict[Tuple[int, int], tuple] = {}      # (batch, k) -> device + pinned result buffers of search()
        self._last_call = None        # (batch, k, cut, through the shadow, workspace) of the last search_device
        # The blocking search() stages queries and results through per-instance buffers (pinned query, device
        # query, cached result buffers, workspaces): one caller at a time.  The reference's ExactIndex.search is
        # read-only and therefore safe under concurrent callers; this lock keeps that property for a threaded server.
        self._lock = threading.RLock()
        self._store = None            # [emb, dewi32, ent32, shadow] storage tensors once the corpus was mutated or reserved
        self.reallocations = 0        # how often the storage grew (reserve / an append beyond the capacity)
        self.i8_codes = None          # int8 copy of an fp32 matrix (enable_int8_shadow): [N, dim] codes ...
        self.i8_scales = None         # ... and one fp32 scale per row
        self._i8_stale = False        # the rows changed since the copy was made: the next approximate search re-quantises
        self.b1_bits = None           # 1-bit copy of an fp32 matrix (enable_binary_shadow): [N, dim / 32] dwords as int32
        self._b1_stale = False        # the rows changed since the copy was made: the next binary search re-binarises

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_host(cls, rows: np.ndarray, dewi: np.ndarray, ht_mean: np.ndarray, hi_mean: np.ndarray,
                  space: str = "cosine", normalize: Optional[bool] = None, device: Optional[str] = None,
                  id_offset: int = 0, chunk_rows: int = 262144) -> "DeviceCorpus":
        """Upload raw fp32 rows and payload columns; normalise on the device (A1/A2).

        Replaces N x ``ExactIndex.add`` + ``build`` (reference backends.py:394-412).  Rows
        are streamed in chunks so that the host never needs a second copy of the matrix.
        """
        torch = _torch()
        lib = nat.load_library()
        dev = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[0] == 0:
            raise ValueError("No embeddings to build index from")
        n, d = rows.shape
        if normalize is None:
            normalize = space == "cosine"
        emb = torch.empty((n, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for s in range(0, n, chunk_rows):
                e = min(n, s + chunk_rows)
                blk = torch.from_numpy(np.ascontiguousarray(rows[s:e], dtype=np.float32))
                emb[s:e].copy_(blk, non_blocking=False)
            if normalize:
                nat.check(lib.dewi_normalize_rows_f32(nat.ptr(emb), nat.ptr(emb), n, d, nat.stream_ptr()))
            cols = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64)).to(dev) for c in (dewi, ht_mean, hi_mean)]
            if any(c.numel() != n for c in cols):
                raise ValueError("payload columns must have one value per row")
            dewi32 = torch.empty(n, dtype=torch.float32, device=dev)
            ent32 = torch.empty(n, dtype=torch.float32, device=dev)
            nat.check(lib.dewi_payload_soa_f64(nat.ptr(cols[0]), nat.ptr(cols[1]), nat.ptr(cols[2]), nat.ptr(dewi32),
                                               nat.ptr(ent32), n, nat.stream_ptr()))
            torch.cuda.current_stream().synchronize()
        return cls(emb, dewi32, ent32, space, id_offset)

    def to_bf16(self) -> "DeviceCorpus":
        """The same shard with the (already normalised) matrix rounded to bf16 (config C3)."""
        torch = _torch()
        out = torch.empty(self.emb.shape, dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._lib.dewi_convert_f32_to_bf16(nat.ptr(self.emb), nat.ptr(out), self.emb.numel(),
                                                         nat.stream_ptr()))
        return DeviceCorpus(out, self.dewi32, self.ent32, self.space, self.id_offset)

    def enable_bf16_shadow(self, single_query: bool = False) -> "DeviceCorpus":
        """Keep a bf16 copy of this fp32 matrix next to it (+50 % memory).  Batches of 2 or more cosine queries then run the
        matrix-core passes over the copy as a PRE-SELECTION — half the bytes, and 256 queries per corpus pass instead of
        32 for larger batches — and re-score the candidates from the fp32 rows with the row kernels' arithmetic
        (``dewi_knn_rerank_f32_shadow``): results equal the one-query search bit for bit.  Every dim % 8 == 0 from 136 to 1536 columns, >= 64 K
        rows; any other shape simply takes the usual path.

        ``single_query=True`` sends one-query searches through the shadow as well (k <= 16: the bf16 row kernel with
        per-workgroup lists long enough for the error band, 0.24 ms instead of 0.43 at 1 M x 768; larger k: the pass with one
        active query, 0.26 ms; same re-scoring, same answers).  Off by default (+50 % memory for a path the plain scan already
        serves at the HBM rate); a query the pass refuses on an adversarial corpus is repaired inside the library call like
        any matrix-core batch (ABI 5)."""
        torch = _torch()
        if self.is_bf16:
            raise ValueError("the corpus is already bf16")
        if self.space != "cosine":
            raise ValueError("the bf16 shadow serves cosine corpora (stored rows of unit norm)")
        if self.shadow is None:
            # the error bound of the pre-selection (2^-8 of ||e|| ||q|| + accumulation) is proven for rows of norm <= 1.0001:
            # the stored form of a cosine corpus.  Checked once (NaN rows — zero embeddings — are fine: they are in every cut and come last in every result).
            worst = float(torch.nan_to_num(torch.linalg.vector_norm(self.emb, dim=1), nan=0.0).max()) if self.n_rows else 0.0
            if worst > 1.0001:
                raise ValueError(f"rows are not normalised (largest norm {worst:.6f}): the bf16 shadow's error bound "
                                 f"does not hold for this matrix")
            out = torch.empty(self.emb.shape, dtype=torch.bfloat16, device=self.device)
            with torch.cuda.device(self.device):
                nat.check(self._lib.dewi_convert_f32_to_bf16(nat.ptr(self.emb), nat.ptr(out), self.emb.numel(), nat.stream_ptr()))
            self.shadow = out
        self.shadow_min_batch = 1 if single_query else 2
        return self

    # ------------------------------------------------------------------ int8 shadow (approximate route)
    def enable_int8_shadow(self) -> "DeviceCorpus":
        """Keep an int8 copy of this fp32 matrix next to it — one byte per element and one fp32 scale per row: +25 % memory —
        for the APPROXIMATE route ``search_approx_device`` (``dewi_quantize_rows_i8``: a symmetric per-row quantisation,
        ``scale = max|x| / 127``).  Cosine, an fp32 main matrix, ``dim % 16 == 0`` up to 4096 columns; anything else raises
        ``ValueError``.  Nothing else changes: every exact search of the corpus runs as before.

        ``remove_rows`` / ``put_rows`` mark the copy stale; the next approximate search re-quantises the WHOLE matrix (one
        pass over the fp32 rows, about the cost of one exact search) — so a mutated corpus and a freshly built one hold the
        same codes bit for bit.  Incremental re-quantisation is not part of this build."""
        check_int8_shape(self.space, self.is_bf16, self.dim)
        with self._lock, _torch().cuda.device(self.device):
            if self.i8_codes is None or self._i8_stale:
                self._quantize_int8()
        return self

    @property
    def has_int8_shadow(self) -> bool:
        return self.i8_codes is not None

    def _quantize_int8(self) -> None:
        torch = _torch()
        n = self.n_rows
        codes = torch.empty((n, self.dim), dtype=torch.int8, device=self.device)
        scales = torch.empty(n, dtype=torch.float32, device=self.device)
        nat.check(self._lib.dewi_quantize_rows_i8(nat.ptr(self.emb), n, self.dim, nat.ptr(codes), nat.ptr(scales),
                                                  nat.stream_ptr()))
        self.i8_codes, self.i8_scales, self._i8_stale = codes, scales, False

    def _int8(self):
        """(codes, scales) of the int8 copy, re-quantised first if the rows changed since it was made."""
        if self.i8_codes is None:
            raise ValueError("this corpus has no int8 shadow: call enable_int8_shadow() (ExactIndex(int8_shadow=True))")
        if self._i8_stale:
            self._quantize_int8()
        return self.i8_codes, self.i8_scales

    def to_int8(self) -> "Int8Corpus":
        """A stand-alone corpus of the codes, the scales and the payload columns only (0.26 x the memory of the fp32 rows):
        it serves ``search_approx_device(rescore=False)`` / ``search_approx(rescore=False)``; everything else on it raises
        ``NotImplementedError``.  The tensors are shared with this corpus's shadow when it has one."""
        check_int8_shape(self.space, self.is_bf16, self.dim)
        with self._lock, _torch().cuda.device(self.device):
            if self.i8_codes is not None:
                codes, scales = self._int8()
            else:
                self._quantize_int8()
                codes, scales = self.i8_codes, self.i8_scales
                self.i8_codes = self.i8_scales = None
        return Int8Corpus(codes, scales, self.dewi32, self.ent32, self.id_offset)

    def candidates_i8_device(self, q_dev, n_candidates: int, out=None, id_offset: Optional[int] = None,
                             batch_pass: Optional[bool] = None):
        """The ``n_candidates`` best rows of every query BY THE INT8 SCORES as candidate records, int32 view
        [B, n_candidates, 4], in ``candidates_device``'s layout and order (``dewi_knn_candidates_i8``).  ``id_offset``:
        default the corpus's.  ``batch_pass``: ``None`` takes the matrix-core pass of 32 queries per read of the codes
        (``dewi_knn_candidates_i8_batch``) where it takes the shape AND either the corpus has at least
        ``I8_BATCH_AUTO_MIN_ROWS`` rows or the batch at least ``I8_BATCH_AUTO_MIN_BATCH`` queries (a few queries over a small
        corpus: its seven launches cost more than the row passes they save) — the same records, bit for bit —,
        ``False`` forces the row passes (four queries per read), ``True`` takes the pass wherever it takes the shape and
        raises ``ValueError`` where it does not."""
        codes, scales = self._int8()
        b, c = int(q_dev.shape[0]), int(n_candidates)
        n = int(codes.shape[0])
        use_pass = False
        if batch_pass is None or batch_pass:
            use_pass = int(self._lib.dewi_knn_i8_batch_workspace_bytes(n, self.dim, b, c)) > 0
            if batch_pass is None and n < I8_BATCH_AUTO_MIN_ROWS and b < I8_BATCH_AUTO_MIN_BATCH:
                use_pass = False
            if batch_pass and not use_pass:
                raise ValueError(f"batch_pass=True: the int8 batch pass does not take {n} rows x {self.dim} columns, "
                                 f"{b} queries, {c} candidates")
        out = self._records_out(b, c, out)
        if use_pass:
            ws = self._cached_workspace(("i8batch", b, c), self._lib.dewi_knn_i8_batch_workspace_bytes, n, self.dim, b, c)
            entry = self._lib.dewi_knn_candidates_i8_batch
        else:
            ws = self._cached_workspace(("i8", b, c), self._lib.dewi_knn_i8_workspace_bytes, n, self.dim, b, c)
            entry = self._lib.dewi_knn_candidates_i8
        nat.check(entry(
            nat.ptr(codes), nat.ptr(scales), n, self.dim, nat.ptr(q_dev), b, nat.ptr(self.dewi32), nat.ptr(self.ent32), c,
            self._record_id_offset(id_offset), nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return out

    # ---- what every ``candidates_*_device`` and every search over candidate records shares
    def _records_out(self, b: int, c: int, out, padded: bool = False):
        """The int32 view [b, c, 4] a ``candidates_*_device`` writes into: the caller's ``out`` or a fresh tensor.  ``padded``
        (the call is going to write nothing): filled with the padding record (sim -inf, dewi 0, ent 0, id -1)."""
        torch = _torch()
        if out is None:
            out = torch.empty((b, c, 4), dtype=torch.int32, device=self.device)
        if padded:
            out.copy_(torch.tensor([-0x800000, 0, 0, -1], dtype=torch.int32, device=self.device).expand(b, c, 4))
        return out

    def _record_id_offset(self, id_offset: Optional[int]) -> int:
        return self.id_offset if id_offset is None else int(id_offset)

    def _rerank_records(self, q_dev, recs, rescore: bool, k: int, eta: float, entropy_pref: float, out_ids, out_scores):
        """The tail of a search over candidate records with LOCAL ids ([B, c, 4] int32 view): re-scored from the fp32 rows
        where ``rescore`` says so, then blended and cut to k (``dewi_merge_rerank``) -> (ids, scores) [B, k]."""
        b, c = int(recs.shape[0]), int(recs.shape[1])
        if rescore:
            self.rescore_candidates_device(q_dev, recs, id_offset=0)
        return merge_rerank_device(recs.view(1, b, c, 4), c, k, eta, entropy_pref, out_ids, out_scores)

    def _blocking(self, search_device, queries: ArrayLike, *args, ids: str = "offset") -> Tuple[np.ndarray, np.ndarray]:
        """The blocking twin of a ``*_device`` search: the queries staged and ``search_device(q, *args)`` run under the
        per-corpus lock, (ids int64, scores fp32) brought to the host.  ``ids``: how they become global — ``"offset"`` adds
        ``id_offset``, ``"offset_valid"`` adds it where the id is not the padding's (-1 stays -1), ``"global"`` leaves them
        (the candidate records already carried global ids)."""
        with self._lock, _torch().cuda.device(self.device):
            ids_d, sc_d = search_device(self.stage_queries(queries), *args)
            ids_h, scores_h = ids_d.cpu().numpy(), sc_d.cpu().numpy()
        if self.id_offset and ids == "offset":
            ids_h = ids_h + self.id_offset
        elif self.id_offset and ids == "offset_valid":
            ids_h = np.where(ids_h >= 0, ids_h + self.id_offset, ids_h)
        return ids_h, scores_h

    def rescore_candidates_device(self, q_dev, recs, id_offset: Optional[int] = None):
        """In place: the similarity of every record of ``recs`` ([B, c, 4] int32 view) becomes the fp32 inner product of its
        stored fp32 row and the normalised query, and each query's list is sorted again (``dewi_rescore_candidates_f32``)."""
        if self.is_bf16:
            raise NotImplementedError("candidates are re-scored from fp32 rows (this corpus is bf16)")
        nat.check(self._lib.dewi_rescore_candidates_f32(
            nat.ptr(self.emb), self.n_rows, self.dim, nat.ptr(q_dev), int(recs.shape[0]), nat.ptr(recs), int(recs.shape[1]),
            self._record_id_offset(id_offset), nat.stream_ptr()))
        return recs

    def search_approx_device(self, q_dev, k: int, eta: float, entropy_pref: float, candidates: Optional[int] = None,
                             rescore: bool = True, out_ids=None, out_scores=None):
        """Enqueue one APPROXIMATE search on the current stream; returns device tensors ``(ids, scores)`` [B, k] (local row
        ids, as ``search_device``), no sync.  The cut — ``min(2k, N)``, or ``candidates`` (up to 1024) — is taken by the int8
        scores of the shadow (a quarter of the fp32 rows' bytes), then — ``rescore=True`` — re-scored from the fp32 rows,
        then blended and cut to k exactly as every search (``dewi_knn_candidates_i8`` -> ``dewi_rescore_candidates_f32`` ->
        ``dewi_merge_rerank``).  With ``rescore`` the returned scores are fp32 similarities' blends; a document is missed
        only when the int8 scores drop it from the cut (recall: DESIGN.md 4.1q).  ``k`` above the cut and a cut above 1024
        raise ``ValueError``.  Batches take the matrix-core pass over the codes where it takes the shape
        (``candidates_i8_device``; the same bits either way — ``search_approx(batch_pass=False)`` is the way back to the row
        passes).  NOT thread-safe on one instance (shared workspaces)."""
        return self._search_approx_device(q_dev, k, eta, entropy_pref, candidates, rescore, out_ids, out_scores, None)

    def _search_approx_device(self, q_dev, k, eta, entropy_pref, candidates, rescore, out_ids, out_scores, batch_pass):
        """``search_approx_device`` with ``candidates_i8_device``'s ``batch_pass``."""
        b, k = check_search_args(q_dev.shape, self.dim, k, None, "ip")
        if k <= 0:
            return empty_result(b, self.device)
        c = approx_cut(k, candidates, self.n_rows)
        recs = self.candidates_i8_device(q_dev, c, id_offset=0, batch_pass=batch_pass)
        return self._rerank_records(q_dev, recs, rescore, k, eta, entropy_pref, out_ids, out_scores)

    def search_approx(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                      candidates: Optional[int] = None, rescore: bool = True,
                      batch_pass: Optional[bool] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking twin of ``search`` for ``search_approx_device``: (ids int64 [B, k] including id_offset, scores fp32
        [B, k]) on the host.  Serialised by the per-corpus lock.  ``batch_pass``: as ``candidates_i8_device`` — ``None``
        takes the matrix-core pass where it takes the shape, ``False`` the row passes, ``True`` insists (``ValueError``)."""
        # (the private twin, NOT self.search_approx_device: the public method's parameter list is pinned and cannot carry
        # batch_pass — a subclass that overrides search_approx_device must override this method too, as Int8Corpus does)
        return self._blocking(self._search_approx_device, queries, k, eta, entropy_pref, candidates, rescore, None, None, batch_pass)

    # ------------------------------------------------------------------ binary shadow (approximate route)
    def enable_binary_shadow(self) -> "DeviceCorpus":
        """Keep a 1-BIT copy of this fp32 matrix next to it — the sign of every element, ``dim / 8`` bytes per row: +3 %
        memory — for the APPROXIMATE route ``search_binary_device`` (``dewi_binarize_rows_f32``).  Cosine, an fp32 main
        matrix, ``dim % 128 == 0`` from 128 to 4096 columns; anything else raises ``ValueError``.  Nothing else changes:
        every other search of the corpus runs as before, and nothing routes here by itself.

        ``remove_rows`` / ``put_rows`` mark the copy stale; the next binary search re-binarises the WHOLE matrix (one pass
        over the fp32 rows) — so a mutated corpus and a freshly built one hold the same bits.  The int8 copy's rule."""
        check_binary_shape(self.space, self.is_bf16, self.dim)
        with self._lock, _torch().cuda.device(self.device):
            if self.b1_bits is None or self._b1_stale:
                self._binarize()
        return self

    @property
    def has_binary_shadow(self) -> bool:
        return self.b1_bits is not None

    def _binarize(self) -> None:
        torch = _torch()
        n = self.n_rows
        bits = torch.empty((n, self.dim // 32), dtype=torch.int32, device=self.device)
        nat.check(self._lib.dewi_binarize_rows_f32(nat.ptr(self.emb), n, self.dim, nat.ptr(bits), nat.stream_ptr()))
        self.b1_bits, self._b1_stale = bits, False

    def _binary(self):
        """The bits of the binary copy, made again first if the rows changed since."""
        if self.b1_bits is None:
            raise ValueError("this corpus has no binary shadow: call enable_binary_shadow() (ExactIndex(binary_shadow=True))")
        if self._b1_stale:
            self._binarize()
        return self.b1_bits

    def candidates_b1_device(self, q_dev, n_candidates: int, out=None, id_offset: Optional[int] = None):
        """The ``n_candidates`` best rows of every RAW query by the HAMMING scores of the binary copy as candidate records,
        int32 view [B, n_candidates, 4], in ``candidates_device``'s layout and order (``dewi_knn_candidates_b1``).
        ``id_offset``: default the corpus's."""
        bits = self._binary()
        b, c = int(q_dev.shape[0]), int(n_candidates)
        n = int(bits.shape[0])
        out = self._records_out(b, c, out)
        ws = self._cached_workspace(("b1", b, c), self._lib.dewi_knn_b1_workspace_bytes, n, self.dim, b, c)
        nat.check(self._lib.dewi_knn_candidates_b1(
            nat.ptr(bits), n, self.dim, nat.ptr(q_dev), b, nat.ptr(self.dewi32), nat.ptr(self.ent32), c,
            self._record_id_offset(id_offset), nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return out

    def search_binary_device(self, q_dev, k: int, eta: float, entropy_pref: float, candidates: Optional[int] = None,
                             rescore: bool = True, out_ids=None, out_scores=None):
        """Enqueue one APPROXIMATE search over the binary copy on the current stream; returns device tensors ``(ids, scores)``
        [B, k] (local row ids, as ``search_device``), no sync.  The cut — ``binary_cut``: ``min(N, 1024, max(128, 16 k))``, or
        ``candidates`` (up to 1024) — is taken by Hamming distance between sign bits (1 / 32 of the fp32 rows' bytes), then —
        ``rescore=True`` — re-scored from the fp32 rows, then blended and cut to k exactly as every search
        (``dewi_knn_candidates_b1`` -> ``dewi_rescore_candidates_f32`` -> ``dewi_merge_rerank``).  ``rescore=False`` blends
        the Hamming similarity ``(dim - 2 h) / dim`` as it is.  A document is missed when the Hamming scores drop it from the
        cut (recall: DESIGN.md 4.1aa).  ``k`` above the cut and a cut above 1024 raise ``ValueError``.  NOT thread-safe on
        one instance (shared workspaces)."""
        b, k = check_search_args(q_dev.shape, self.dim, k, None, "ip")
        if k <= 0:
            return empty_result(b, self.device)
        self._binary()
        c = binary_cut(k, candidates, self.n_rows)
        recs = self.candidates_b1_device(q_dev, c, id_offset=0)
        return self._rerank_records(q_dev, recs, rescore, k, eta, entropy_pref, out_ids, out_scores)

    def search_binary(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                      candidates: Optional[int] = None, rescore: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking twin of ``search`` for ``search_binary_device``: (ids int64 [B, k] including id_offset, scores fp32
        [B, k]) on the host.  Serialised by the per-corpus lock."""
        return self._blocking(self.search_binary_device, queries, k, eta, entropy_pref, candidates, rescore)

    # ------------------------------------------------------------------ approximate route over allow-lists
    def candidates_i8_filtered_device(self, q_dev, n_candidates: int, filter, out=None, id_offset: Optional[int] = None):
        """``candidates_i8_device`` over the rows of ``filter`` only: a ``DeviceFilter`` of this corpus (one list for every
        query: ``dewi_knn_candidates_i8_filtered``) or a ``DeviceQueryFilters`` of B lists, every one of them at least
        ``n_candidates`` long (``dewi_knn_candidates_i8_query_filtered``; shorter lists are the caller's split).  Ids are rows
        of the whole corpus.  An empty ``DeviceFilter`` writes nothing: ``out`` is returned filled with padding."""
        codes, scales = self._int8()
        b, c = int(q_dev.shape[0]), int(n_candidates)
        n = int(codes.shape[0])
        off = self._record_id_offset(id_offset)
        if isinstance(filter, DeviceQueryFilters):
            self.check_query_filters(filter, b)
            out = self._records_out(b, c, out)
            ws = self._cached_workspace(("i8qf", b, filter.n_union, c), self._lib.dewi_knn_i8_filtered_workspace_bytes,
                                        filter.n_union, self.dim, b, c)
            n_a = (ctypes.c_int64 * b)(*[int(x) for x in filter.n_allowed])
            nat.check(self._lib.dewi_knn_candidates_i8_query_filtered(
                nat.ptr(codes), nat.ptr(scales), n, self.dim, nat.ptr(filter.buf), filter.n_union, n_a, nat.ptr(q_dev), b,
                nat.ptr(self.dewi32), nat.ptr(self.ent32), c, off, nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
            return out
        self.check_filter(filter)
        out = self._records_out(b, c, out, padded=filter.n_allowed == 0)
        if filter.n_allowed == 0:
            return out
        ws = self._cached_workspace(("i8f", b, filter.n_allowed, c), self._lib.dewi_knn_i8_filtered_workspace_bytes,
                                    filter.n_allowed, self.dim, b, c)
        nat.check(self._lib.dewi_knn_candidates_i8_filtered(
            nat.ptr(codes), nat.ptr(scales), n, self.dim, nat.ptr(filter.buf), filter.n_allowed, nat.ptr(q_dev), b,
            nat.ptr(self.dewi32), nat.ptr(self.ent32), c, off, nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return out

    def _approx_one_list(self, q_dev, k: int, eta: float, entropy_pref: float, candidates: Optional[int], rescore: bool,
                         f: DeviceFilter, out_ids, out_scores):
        recs = self.candidates_i8_filtered_device(q_dev, approx_cut(k, candidates, f.n_allowed), f, id_offset=0)
        return self._rerank_records(q_dev, recs, rescore, k, eta, entropy_pref, out_ids, out_scores)

    def search_approx_filtered_device(self, q_dev, k: int, eta: float, entropy_pref: float, filter,
                                      candidates: Optional[int] = None, rescore: bool = True, out_ids=None, out_scores=None):
        """``search_approx_device`` over the rows of ``filter`` only (a ``DeviceFilter`` or a ``DeviceQueryFilters`` of this
        corpus; stale filters raise ``ValueError``): the cut ``approx_cut(k, candidates, |A|)`` is taken by the int8 scores of
        the listed rows — a quarter of the bytes ``search_device(filter=)`` reads —, re-scored from the fp32 rows unless
        ``rescore=False``, then blended and cut to k.  Local row ids, no sync.  ``k`` above ``|A|`` raises ``ValueError``; an
        empty ``DeviceFilter`` gives [B, 0].  ``DeviceQueryFilters``: the host split of ``search_device``: lists at least as
        long as the cut share one pass over the union, a shorter list runs on a filter of its own (its cut is ``|F_j|``), an
        empty list leaves id -1 / score NaN in its row."""
        if isinstance(filter, DeviceQueryFilters):
            qf = filter
            self.check_query_filters(qf, int(q_dev.shape[0]))
        else:
            self.check_filter(filter)
        b, k = check_search_args(q_dev.shape, self.dim, k, None, "ip")
        self._int8()
        if k <= 0:
            return empty_result(b, self.device)
        if not isinstance(filter, DeviceQueryFilters):
            if filter.n_allowed == 0:
                return empty_result(b, self.device)
            if k > filter.n_allowed:
                raise ValueError(f"k = {k} exceeds the {filter.n_allowed} rows the filter allows")
            return self._approx_one_list(q_dev, k, eta, entropy_pref, candidates, rescore, filter, out_ids, out_scores)
        counts = qf.n_allowed
        for j in range(b):
            if 0 < counts[j] < k:
                raise ValueError(f"query {j}: k = {k} exceeds the {int(counts[j])} rows its filter allows")
        c = approx_cut(k, candidates, self.n_rows)
        out_ids, out_scores = default_outputs(b, k, self.device, out_ids, out_scores)

        def run_shared(sub, q_sub, o_ids, o_sc):
            recs = self.candidates_i8_filtered_device(q_sub, c, sub, id_offset=0)
            self._rerank_records(q_sub, recs, rescore, k, eta, entropy_pref, o_ids, o_sc)

        def run_single(f, q_1, o_ids, o_sc):
            self._approx_one_list(q_1, k, eta, entropy_pref, candidates, rescore, f, o_ids, o_sc)

        return self._split_query_lists(qf, q_dev, k, c, out_ids, out_scores, run_shared, run_single)

    def search_approx_filtered(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *, filter,
                               candidates: Optional[int] = None, rescore: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking twin of ``search_approx_filtered_device``: (ids int64 [B, k] including id_offset — -1 stays -1 —, scores
        fp32 [B, k]) on the host.  Serialised by the per-corpus lock."""
        return self._blocking(self.search_approx_filtered_device, queries, k, eta, entropy_pref, filter, candidates, rescore,
                              ids="offset_valid")

    # ------------------------------------------------------------------ properties
    @property
    def n_rows(self) -> int:
        return int(self.emb.shape[0])

    @property
    def dim(self) -> int:
        return int(self.emb.shape[1])

    @property
    def is_bf16(self) -> bool:
        return self.emb.dtype == _torch().bfloat16

    @property
    def _elem(self) -> int:
        """``elem_type`` of the ABI: 0 fp32, 1 bf16."""
        return 1 if self.is_bf16 else 0

    def corpus_bytes(self) -> int:
        return self.emb.numel() * self.emb.element_size()

    # ------------------------------------------------------------------ mutation (additive; the reference only rebuilds)
    @property
    def capacity(self) -> int:
        """Rows the storage holds without reallocating; ``n_rows`` for a corpus built as ever."""
        return self.n_rows if self._store is None else int(self._store[0].shape[0])

    def _stores(self):
        """[emb, dewi32, ent32, shadow or None]: the storage tensors whose first ``n_rows`` rows are the corpus."""
        st = self._store
        if st is None:
            st = self._store = [self.emb, self.dewi32, self.ent32, self.shadow]
        if self.shadow is not None and (st[3] is None or int(st[3].shape[0]) < int(st[0].shape[0])):
            sh = self.shadow                   # enabled after the storage was made: give it the storage's capacity
            if int(sh.shape[0]) < int(st[0].shape[0]):
                sh = _torch().empty((int(st[0].shape[0]), self.dim), dtype=sh.dtype, device=self.device)
                sh[: self.n_rows].copy_(self.shadow)
            st[3] = sh
            self.shadow = sh[: self.n_rows]
        return st

    def _set_rows(self, n: int) -> None:
        st = self._stores()
        self.emb, self.dewi32, self.ent32 = st[0][:n], st[1][:n], st[2][:n]
        if st[3] is not None:
            self.shadow = st[3][:n]

    def _grow(self, rows: int) -> None:
        torch = _torch()
        n = self.n_rows
        old = self._stores()
        new = []
        for t in old:
            if t is None:
                new.append(None)
                continue
            g = torch.empty((int(rows),) + tuple(t.shape[1:]), dtype=t.dtype, device=self.device)
            g[:n].copy_(t[:n])
            new.append(g)
        self._store = new
        self._set_rows(n)
        self.reallocations += 1

    def reserve(self, rows: int) -> None:
        """Make room for ``rows`` rows: the matrix, the shadow and the payload columns become prefixes (``storage[:n]``, still
        contiguous) of storage tensors of that many rows, so later appends up to there do not reallocate.  Growth is a
        device-to-device copy into new tensors: peak memory is the old storage plus the new, and a caller's tensor the
        build adopted in place (device-resident ingest) is no longer aliased afterwards.  The content does not change, so
        prepared filters stay valid; a ``PipelinedSearcher`` made before holds the old pointers and must be made again.
        The storage never shrinks."""
        with self._lock, _torch().cuda.device(self.device):
            self._check_mutable()
            if int(rows) > self.capacity:
                self._grow(int(rows))

    def _check_mutable(self) -> None:
        if self.is_bf16:
            raise NotImplementedError("in-place mutation serves fp32 corpora (a bf16 main matrix: not in this build)")

    def _after_mutation(self) -> None:
        """The corpus is another one now: filters prepared before are refused, cached workspaces and result buffers go."""
        self.corpus_id = next(_corpus_ids)
        self._ws.clear()
        self._io.clear()
        self._last_call = None
        if self.i8_codes is not None:
            self._i8_stale = True              # re-quantised as a whole by the next approximate search (_int8)
        if self.b1_bits is not None:
            self._b1_stale = True              # re-binarised as a whole by the next binary search (_binary)

    def _read_error(self, err, what: str) -> None:
        bad = int(err.item())                  # the call's one synchronisation
        if bad:
            raise nat.NativeLibraryError(f"{what}: {bad} rows outside the contract were skipped (corpus state is undefined)")

    def remove_rows(self, rows, aux=None) -> Tuple[np.ndarray, np.ndarray]:
        """Delete ``rows`` in place (``plan_remove``: the tail fills the holes) and return the ``(src, dst)`` pairs applied;
        the corpus then has ``n_rows - len(rows)`` rows.  One ``dewi_rows_move`` launch on the current stream moves the
        matrix rows, the shadow rows, both payload columns and ``aux`` (an int32 device tensor of one word per row, e.g. the
        IVF cells; the caller cuts it to the new ``n_rows``) together; the error word is read once (one synchronisation).
        Afterwards the corpus has a new ``corpus_id`` — filters prepared before raise ``ValueError`` — and the cached
        workspaces and result buffers are dropped.  The storage keeps its capacity.  fp32 corpora; the payload columns of a
        ``to_bf16()`` copy made before alias this corpus's and are not kept consistent."""
        torch = _torch()
        with self._lock, torch.cuda.device(self.device):
            self._check_mutable()
            n = self.n_rows
            src, dst, n_keep = plan_remove(n, rows)
            if n_keep == n:
                return src, dst
            if aux is not None:
                assert aux.is_cuda and aux.dtype == torch.int32 and aux.is_contiguous() and int(aux.numel()) >= n
            st = self._stores()
            if src.size:
                pairs = torch.from_numpy(np.stack([src, dst])).to(self.device)
                err = torch.zeros(1, dtype=torch.int32, device=self.device)
                nat.check(self._lib.dewi_rows_move(
                    nat.ptr(st[0]), 0, nat.ptr(st[3]), nat.ptr(st[1]), nat.ptr(st[2]), nat.ptr(aux), n, self.dim, n_keep,
                    nat.ptr(pairs[0]), nat.ptr(pairs[1]), int(src.size), nat.ptr(err), nat.stream_ptr()))
                self._read_error(err, "dewi_rows_move")
            self._set_rows(n_keep)
            self._after_mutation()
            return src, dst

    def put_rows(self, rows, raw, dewi, ht_mean, hi_mean, normalize: Optional[bool] = None) -> int:
        """Write raw embeddings and payloads into ``rows`` — existing rows (replaced in place) and/or exactly the next ``a``
        rows ``n_rows .. n_rows + a - 1`` (appended) — and return ``a``.  ``raw``: [m, dim], a host array or a CUDA fp32
        tensor; ``dewi`` / ``ht_mean`` / ``hi_mean``: [m] float64 values, host or device.  One ``dewi_rows_put_f32`` launch
        on the current stream stores what a fresh build stores for these rows, bit for bit (``normalize``: default for
        ``space="cosine"``), shadow and payload columns included; the error word is read once.  An append beyond the
        capacity first grows the storage to ``max(needed, capacity + capacity // CAPACITY_GROWTH_DIVISOR)`` (see
        ``reserve``).  Afterwards: a new ``corpus_id``, no cached workspaces, as ``remove_rows``."""
        torch = _torch()
        with self._lock, torch.cuda.device(self.device):
            self._check_mutable()
            n = self.n_rows
            r = np.asarray(rows).reshape(-1)
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise ValueError(f"rows to put must be integers, got {r.dtype}")
            r = np.ascontiguousarray(r, dtype=np.int64)
            m = int(r.size)
            if m == 0:
                return 0
            new = np.sort(r[r >= n])
            a = int(new.size)
            if int(r.min()) < 0 or np.unique(r).size != m or not np.array_equal(new, np.arange(n, n + a)):
                raise ValueError(f"rows to put must be distinct rows of [0, {n}) and/or exactly the next rows from {n} on")
            if isinstance(raw, torch.Tensor):
                x = raw.to(device=self.device, dtype=torch.float32).contiguous()
            else:
                x = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).to(self.device)
            if x.dim() != 2 or tuple(x.shape) != (m, self.dim):
                raise ValueError(f"Expected embeddings of shape ({m}, {self.dim}), got {tuple(x.shape)}")
            cols = [(c.to(device=self.device, dtype=torch.float64) if isinstance(c, torch.Tensor)
                     else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64)).to(self.device)).reshape(-1).contiguous()
                    for c in (dewi, ht_mean, hi_mean)]
            if any(int(c.numel()) != m for c in cols):
                raise ValueError("payload columns must have one value per row")
            if normalize is None:
                normalize = self.space == "cosine"
            need = n + a
            if need > self.capacity:
                self._grow(max(need, self.capacity + self.capacity // CAPACITY_GROWTH_DIVISOR))
            st = self._stores()
            slots = torch.from_numpy(r).to(self.device)
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            nat.check(self._lib.dewi_rows_put_f32(
                nat.ptr(st[0]), nat.ptr(st[3]), nat.ptr(st[1]), nat.ptr(st[2]), need, self.dim, 1 if normalize else 0,
                nat.ptr(x), nat.ptr(cols[0]), nat.ptr(cols[1]), nat.ptr(cols[2]), nat.ptr(slots), m, nat.ptr(err),
                nat.stream_ptr()))
            self._read_error(err, "dewi_rows_put_f32")
            self._set_rows(need)
            self._after_mutation()
            return a

    # ------------------------------------------------------------------ helpers
    def _cached_workspace(self, key, size_fn, *size_args):
        """The workspace of every entry point of this corpus: one tensor per ``key``.  The required size depends on the launch
        plan (tunable), so an entry is good for the tuning it was sized under: a hit under the calling thread's current
        tuning costs one lookup; otherwise ``size_fn(*size_args)`` asks the library again (it plans every path of the shape —
        a few microseconds that a 40 us search need not pay each time) and the tensor grows if the size did.  More than 8
        entries: the cache is dropped before the next allocation.  An entry holds ONE epoch: two threads under different
        tunings that share a corpus and a key re-ask the size on every call (correct — the tensor only grows — and
        ``search_device`` is one caller at a time per instance anyway); a size per thread was not worth a second table."""
        epoch = getattr(_thread_tuning, "epoch", 0)
        hit = self._ws.get(key)
        if hit is not None and hit[1] == epoch:
            return hit[0]
        need = library_size(size_fn, *size_args)
        ws = None if hit is None else hit[0]
        if ws is None or ws.numel() < need:
            if len(self._ws) > 8:
                self._ws.clear()
            ws = _torch().empty(need, dtype=_torch().uint8, device=self.device)
        self._ws[key] = (ws, epoch)
        return ws

    def cached_workspaces(self) -> Dict[tuple, "torch.Tensor"]:  # noqa: F821
        """Tests / diagnostics: key -> workspace tensor of every entry ``_cached_workspace`` holds (a copy of the table)."""
        return {key: hit[0] for key, hit in self._ws.items()}

    def replace_cached_workspace(self, key, ws) -> None:
        """Tests: put ``ws`` (uint8, at least as large as the entry it replaces) under ``key``, keeping the tuning epoch the
        entry was sized under — the next call under that tuning runs in ``ws`` without asking the size again."""
        old, epoch = self._ws[key]
        if ws.numel() < old.numel():
            raise ValueError(f"workspace {key}: {ws.numel()} bytes replace {old.numel()}")
        self._ws[key] = (ws, epoch)

    def drop_cached_workspaces(self) -> None:
        """Tests: forget every cached workspace (the next call of each shape allocates afresh)."""
        self._ws.clear()

    def _workspace(self, n_queries: int, n_candidates: int):
        return self._cached_workspace((n_queries, n_candidates), self._lib.dewi_knn_workspace_bytes, self.n_rows, self.dim,
                                      n_queries, n_candidates)

    def stage_queries(self, queries: ArrayLike):
        """Host or device query batch -> contiguous fp32 [B, d] tensor on this device."""
        torch = _torch()
        if isinstance(queries, torch.Tensor):
            q = queries
            if q.dim() == 1:
                q = q.unsqueeze(0)
            return q.to(device=self.device, dtype=torch.float32).contiguous()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        q = np.ascontiguousarray(q)
        if self._q_pinned is None or self._q_pinned.shape != q.shape:
            self._q_pinned = torch.empty(q.shape, dtype=torch.float32, pin_memory=True)
            self._q_pinned_np = self._q_pinned.numpy()
            self._q_dev = torch.empty(q.shape, dtype=torch.float32, device=self.device)
        self._q_pinned_np[...] = q
        self._q_dev.copy_(self._q_pinned, non_blocking=True)
        return self._q_dev

    # ------------------------------------------------------------------ filters
    def make_filter(self, mask) -> DeviceFilter:
        """Prepare an allow-list from a bool mask of length N (numpy or torch, host or device).  Synchronises the current
        stream once (the count of allowed rows comes back to the host)."""
        torch = _torch()
        if isinstance(mask, torch.Tensor):
            m = mask
        else:
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
        if m.dim() != 1 or int(m.shape[0]) != self.n_rows:
            raise ValueError(f"filter mask must have shape ({self.n_rows},), got {tuple(m.shape)}")
        if m.dtype != torch.bool:
            raise ValueError(f"filter mask must be boolean, got {m.dtype}")
        elem = self._elem
        need = library_size(self._lib.dewi_filter_bytes, self.n_rows, self.dim, elem)
        with torch.cuda.device(self.device):
            m8 = m.to(device=self.device).view(torch.uint8).contiguous()
            buf = torch.empty(need, dtype=torch.uint8, device=self.device)
            n_allowed = ctypes.c_int64(0)
            nat.check(self._lib.dewi_filter_prepare(elem, self.n_rows, self.dim, nat.ptr(m8), nat.ptr(buf), need,
                                                    ctypes.byref(n_allowed), nat.stream_ptr()))
        return DeviceFilter(buf, n_allowed.value, self.corpus_id, self.n_rows)

    def check_filter(self, filter: DeviceFilter) -> None:
        if not isinstance(filter, DeviceFilter):
            raise TypeError(f"expected a DeviceFilter (make_filter), got {type(filter).__name__}")
        if filter.corpus_id != self.corpus_id:
            raise ValueError("this filter was prepared for another corpus (the index was rebuilt or reloaded since): "
                             "prepare it again with make_filter")

    def make_query_filters(self, masks) -> DeviceQueryFilters:
        """Prepare per-query allow-lists from a bool mask of shape [B, N] (numpy or torch, host or device): row j is the
        list of query j of the batches this set serves.  Synchronises the current stream once (|U| and every |F_j| come
        back to the host)."""
        torch = _torch()
        if isinstance(masks, torch.Tensor):
            m = masks
        else:
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(masks)))
        if m.dim() != 2 or int(m.shape[1]) != self.n_rows or int(m.shape[0]) < 1:
            raise ValueError(f"query filter masks must have shape (B, {self.n_rows}) with B >= 1, got {tuple(m.shape)}")
        if m.dtype != torch.bool:
            raise ValueError(f"query filter masks must be boolean, got {m.dtype}")
        b = int(m.shape[0])
        elem = self._elem
        need = library_size(self._lib.dewi_query_filter_bytes, self.n_rows, self.dim, elem, b)
        with torch.cuda.device(self.device):
            m8 = m.to(device=self.device).view(torch.uint8).contiguous()
            buf = torch.empty(need, dtype=torch.uint8, device=self.device)
            n_union = ctypes.c_int64(0)
            counts = (ctypes.c_int64 * b)()
            nat.check(self._lib.dewi_query_filter_prepare(elem, self.n_rows, self.dim, b, nat.ptr(m8), nat.ptr(buf), need,
                                                          ctypes.byref(n_union), counts, nat.stream_ptr()))
        return DeviceQueryFilters(buf, m8, np.frombuffer(counts, dtype=np.int64).copy(), n_union.value, self.corpus_id,
                                  self.n_rows)

    # ------------------------------------------------------------------ predicates over attribute columns
    def predicate_masks(self, columns, programs, sets, base=None):
        """Evaluate postfix predicate programs (``dewi.where``; ``dewi_predicate_masks``) over attribute columns of this corpus:
        ``columns`` device tensors [n_rows] of int32 or float32, ``programs`` P lists of ``(op, column, a, b)``, ``sets`` the
        uint32 words of the ``isin`` bitsets (numpy or device), ``base`` ``None`` or device bytes / bools [n_rows] ANDed into
        every result.  Returns a device uint8 tensor [P, n_rows] of 0 / 1.  Asynchronous on the current stream: no
        synchronisation, no workspace."""
        torch = _torch()
        n = self.n_rows
        cols = list(columns)
        types = (ctypes.c_int32 * max(len(cols), 1))()
        ptrs = (ctypes.c_void_p * max(len(cols), 1))()
        for i, c in enumerate(cols):
            if not (isinstance(c, torch.Tensor) and c.is_cuda and c.dim() == 1 and int(c.shape[0]) == n and c.is_contiguous()
                    and c.dtype in (torch.int32, torch.float32)):
                raise ValueError(f"attribute column {i} must be a contiguous CUDA int32 / float32 tensor of shape ({n},)")
            types[i] = 1 if c.dtype == torch.float32 else 0
            ptrs[i] = c.data_ptr()
        progs = [list(p) for p in programs]
        n_instr = sum(len(p) for p in progs)
        instr = (nat.PredInstr * max(n_instr, 1))()
        lengths = (ctypes.c_int32 * max(len(progs), 1))()
        at = 0
        for j, p in enumerate(progs):
            lengths[j] = len(p)
            for op, c, a, b in p:
                instr[at] = nat.PredInstr(int(op), int(c), int(a) & 0xFFFFFFFF, int(b) & 0xFFFFFFFF)
                at += 1
        with torch.cuda.device(self.device):
            if isinstance(sets, torch.Tensor):
                s = sets.to(device=self.device).contiguous()
                assert s.dtype == torch.int32
            else:
                s = torch.from_numpy(np.ascontiguousarray(sets, dtype=np.uint32).view(np.int32)).to(self.device)
            b8 = None
            if base is not None:
                if tuple(base.shape) != (n,) or base.dtype not in (torch.uint8, torch.bool):
                    raise ValueError(f"base mask must be bytes or bools of shape ({n},)")
                b8 = base.to(device=self.device).view(torch.uint8).contiguous()
            out = torch.empty((len(progs), n), dtype=torch.uint8, device=self.device)
            nat.check(self._lib.dewi_predicate_masks(ptrs, types, len(cols), n, instr, lengths, len(progs),
                                                     nat.ptr(s) if s.numel() else None, int(s.numel()), nat.ptr(b8),
                                                     nat.ptr(out), nat.stream_ptr()))
        return out

    # ------------------------------------------------------------------ facets over attribute columns
    def facet_device(self, keys, key_kind: int, n_bins: int, key_lo: int = 0, edges=None, masks=None, lists=None, values=None):
        """``dewi_facet_run`` over a key column of this corpus: ``keys`` a contiguous CUDA int32 / float32 tensor [n_rows];
        ``edges`` ``None`` (an integer range from ``key_lo``) or ``n_bins + 1`` edges of the keys' dtype (numpy or device);
        the selections — neither ``masks`` nor ``lists``: all rows; ``masks``: device bytes / bools [P, n_rows]; ``lists``:
        ``(lims int64 [P + 1], rows int64 [T])`` on the device, LOCAL rows —; ``values``: ``None`` or a CUDA int32 / float32
        column [n_rows].  Returns device tensors ``(counts int64 [P, n_bins + 2], stats)``, ``stats`` ``None`` or a dict
        ``vcount`` / ``vmin`` / ``vmax`` / ``vsum``.  Asynchronous on the current stream: no synchronisation."""
        torch = _torch()
        n = self.n_rows

        def column(t, what):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 1 and int(t.shape[0]) == n and t.is_contiguous()
                    and t.dtype in (torch.int32, torch.float32)):
                raise ValueError(f"{what} must be a contiguous CUDA int32 / float32 tensor of shape ({n},)")
            return t

        keys = column(keys, "the key column")
        if (keys.dtype == torch.float32) != (key_kind == nat.FACET_KEY_CODES["f32_edges"]):
            raise ValueError(f"key kind {key_kind} does not take a {keys.dtype} column")
        if masks is not None and lists is not None:
            raise ValueError("pass masks or lists, not both")
        vt = nat.FACET_VALUE_CODES[None]
        if values is not None:
            values = column(values, "the value column")
            vt = nat.FACET_VALUE_CODES["float" if values.dtype == torch.float32 else "int"]
        with torch.cuda.device(self.device):
            e = None
            if edges is not None:
                e = edges if isinstance(edges, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(edges))
                e = e.to(device=self.device, dtype=keys.dtype).contiguous()
                if tuple(e.shape) != (int(n_bins) + 1,):
                    raise ValueError(f"{n_bins} bins take {int(n_bins) + 1} edges, got {tuple(e.shape)}")
            sel, p, m8, lims, rows, t = nat.FACET_SEL_CODES["all"], 1, None, None, None, 0
            if masks is not None:
                if masks.dim() != 2 or int(masks.shape[1]) != n or masks.dtype not in (torch.uint8, torch.bool):
                    raise ValueError(f"selection masks must be bytes or bools of shape (P, {n})")
                m8 = masks.to(device=self.device).view(torch.uint8).contiguous()
                sel, p = nat.FACET_SEL_CODES["masks"], int(m8.shape[0])
            elif lists is not None:
                lims = lists[0].to(device=self.device, dtype=torch.int64).contiguous()
                rows = lists[1].to(device=self.device, dtype=torch.int64).contiguous()
                sel, p, t = nat.FACET_SEL_CODES["lists"], int(lims.shape[0]) - 1, int(rows.shape[0])
                if t == 0:                      # (an empty tensor has no address; the call reads none of it)
                    rows = torch.zeros(1, dtype=torch.int64, device=self.device)
            slots = int(n_bins) + 2
            ws = self._cached_workspace(("facet", int(n_bins), p, vt), self._lib.dewi_facet_workspace_bytes, int(n_bins), p, vt)
            counts = torch.empty((p, slots), dtype=torch.int64, device=self.device)
            stats = None
            if vt:
                stats = {"vcount": torch.empty((p, slots), dtype=torch.int64, device=self.device),
                         "vmin": torch.empty((p, slots), dtype=values.dtype, device=self.device),
                         "vmax": torch.empty((p, slots), dtype=values.dtype, device=self.device),
                         "vsum": torch.empty((p, slots), dtype=torch.float64 if vt == 2 else torch.int64, device=self.device)}
            nat.check(self._lib.dewi_facet_run(
                nat.ptr(keys), int(key_kind), n, int(key_lo), nat.ptr(e) if e is not None else None, int(n_bins), sel, p,
                nat.ptr(m8) if m8 is not None else None, nat.ptr(rows) if rows is not None else None,
                nat.ptr(lims) if lims is not None else None, t, nat.ptr(values) if vt else None, vt, nat.ptr(counts),
                nat.ptr(stats["vcount"]) if vt else None, nat.ptr(stats["vmin"]) if vt else None,
                nat.ptr(stats["vmax"]) if vt else None, nat.ptr(stats["vsum"]) if vt else None, nat.ptr(ws), ws.numel(),
                nat.stream_ptr()))
        return counts, stats

    def make_filter_bytes(self, mask8) -> DeviceFilter:
        """``make_filter`` of a device byte mask [n_rows] of 0 / 1 that this corpus made itself (``predicate_masks``): no copy,
        and the filter's ``byte_mask()`` is seeded with the mask."""
        f = self.make_filter(mask8.view(_torch().bool))
        f._mask = mask8
        return f

    def check_query_filters(self, qf: DeviceQueryFilters, n_queries: Optional[int] = None) -> None:
        if not isinstance(qf, DeviceQueryFilters):
            raise TypeError(f"expected DeviceQueryFilters (make_query_filters), got {type(qf).__name__}")
        if qf.corpus_id != self.corpus_id:
            raise ValueError("these query filters were prepared for another corpus (the index was rebuilt or reloaded "
                             "since): prepare them again with make_query_filters")
        if n_queries is not None and qf.n_queries != n_queries:
            raise ValueError(f"query filters hold {qf.n_queries} lists for a batch of {n_queries} queries")

    def _search_query_filtered(self, q_dev, k: int, eta: float, entropy_pref: float, out_ids, out_scores,
                               candidates: Optional[int], similarity: str, qf: DeviceQueryFilters):
        """``search_device`` where query j searches only its own list F_j.  Queries with |F_j| >= c (c = 2k, or
        ``candidates``) share one pass of the QMASK row kernels over the union (``dewi_knn_rerank_query_filtered``); a
        query with 0 < |F_j| < c runs the one-list search on a filter of its own list (its cut is |F_j|); an empty list
        gives id -1 / score NaN in that query's row.  Every query's result is bit-equal to its one-list search."""
        self.check_query_filters(qf, int(q_dev.shape[0]))
        b, k = check_search_args(q_dev.shape, self.dim, k, candidates, similarity)
        if self.is_bf16:
            raise NotImplementedError("filtered search serves fp32 corpora (bf16: not in this build)")
        if k <= 0:
            return empty_result(b, self.device)
        counts = qf.n_allowed
        for j in range(b):
            if 0 < counts[j] < k:
                raise ValueError(f"query {j}: kth(={int(counts[j]) - k}) out of bounds ({int(counts[j])}): k = {k} exceeds "
                                 f"the {int(counts[j])} rows its filter allows")
        out_ids, out_scores = default_outputs(b, k, self.device, out_ids, out_scores)
        c = cut_size(k, candidates)

        def run_shared(sub, q_sub, o_ids, o_sc):
            nb = int(q_sub.shape[0])
            ws = self._cached_workspace(("qfiltered", nb, sub.n_union, c), self._lib.dewi_knn_query_filtered_workspace_bytes,
                                        sub.n_union, self.dim, nb, c)
            self._last_call = (nb, k, c, False, ws)
            n_a = (ctypes.c_int64 * nb)(*[int(x) for x in sub.n_allowed])
            nat.check(self._lib.dewi_knn_rerank_query_filtered(
                nat.ptr(self.emb), 0, self.n_rows, self.dim, nat.ptr(sub.buf), sub.n_union, n_a, nat.ptr(q_sub), nb,
                nat.ptr(self.dewi32), nat.ptr(self.ent32), k, 0 if candidates is None else int(candidates),
                nat.SIM_CODES[similarity], float(eta), float(entropy_pref), nat.SPACE_CODES[self.space], nat.ptr(o_ids),
                nat.ptr(o_sc), nat.ptr(ws), ws.numel(), nat.stream_ptr()))

        def run_single(f, q_1, o_ids, o_sc):
            self._search_filtered(q_1, k, eta, entropy_pref, o_ids, o_sc, candidates, similarity, f)

        return self._split_query_lists(qf, q_dev, k, c, out_ids, out_scores, run_shared, run_single)

    def _split_query_lists(self, qf: DeviceQueryFilters, q_dev, k: int, c: int, out_ids, out_scores, run_shared, run_single):
        """The host split of a batch whose every query has a list of its own, into ``out_ids`` / ``out_scores`` [B, k].  The
        lists at least as long as the cut ``c`` share one pass: ``run_shared(filters, queries, ids, scores)``, on ``qf`` itself
        when every list is that long, else on the sub-filter of those lists (kept in ``qf._subsets``: cleared when it holds
        more than 8) with outputs of its own that are copied back.  A shorter list runs alone: ``run_single(filter, query
        [1, d], ids [1, k], scores [1, k])`` on the filter of that list (kept in ``qf._singles``).  An empty list leaves the
        padding, id -1 / score NaN, in its row."""
        torch = _torch()
        counts = qf.n_allowed
        b = int(q_dev.shape[0])
        shared = [j for j in range(b) if counts[j] >= c]
        if len(shared) < b:
            out_ids.fill_(-1)
            out_scores.fill_(float("nan"))
        if shared and len(shared) == b:
            run_shared(qf, q_dev, out_ids, out_scores)
        elif shared:
            key = tuple(shared)
            sub = qf._subsets.get(key)
            if sub is None:
                if len(qf._subsets) > 8:
                    qf._subsets.clear()
                sub = qf._subsets[key] = self.make_query_filters(qf.masks[list(shared)].view(torch.bool))
            q_sub = q_dev[shared].contiguous()
            o_ids, o_sc = default_outputs(len(shared), k, self.device)
            run_shared(sub, q_sub, o_ids, o_sc)
            idx = torch.tensor(shared, dtype=torch.int64, device=self.device)
            out_ids.index_copy_(0, idx, o_ids)
            out_scores.index_copy_(0, idx, o_sc)
        for j in range(b):
            if 0 < counts[j] < c:          # a short list: on a filter of its own (its cut is |F_j|)
                f = qf._singles.get(j)
                if f is None:
                    f = qf._singles[j] = self.make_filter(qf.masks[j].view(torch.bool))
                run_single(f, q_dev[j:j + 1], out_ids[j:j + 1], out_scores[j:j + 1])
        return out_ids, out_scores

    def _search_filtered(self, q_dev, k: int, eta: float, entropy_pref: float, out_ids, out_scores,
                         candidates: Optional[int], similarity: str, filter: DeviceFilter):
        """``search_device`` over the rows of a prepared filter (``dewi_knn_rerank_filtered``): the row kernels of this
        dim over the list, then the same select / blend / top-k.  k <= 0 or an empty filter: empty results."""
        self.check_filter(filter)
        b, k = check_search_args(q_dev.shape, self.dim, k, candidates, similarity)
        n_a = filter.n_allowed
        if k <= 0 or n_a == 0:
            return empty_result(b, self.device)
        out_ids, out_scores = default_outputs(b, k, self.device, out_ids, out_scores)
        c = cut_size(k, candidates, n_a)
        ws = self._cached_workspace(("filtered", b, n_a, c), self._lib.dewi_knn_filtered_workspace_bytes, n_a, self.dim, b, c)
        self._last_call = (b, k, c, False, ws)
        rc = self._lib.dewi_knn_rerank_filtered(
            nat.ptr(self.emb), self._elem, self.n_rows, self.dim, nat.ptr(filter.buf), n_a, nat.ptr(q_dev), b,
            nat.ptr(self.dewi32), nat.ptr(self.ent32), k, 0 if candidates is None else int(candidates), nat.SIM_CODES[similarity],
            float(eta), float(entropy_pref), nat.SPACE_CODES[self.space], nat.ptr(out_ids), nat.ptr(out_scores), nat.ptr(ws),
            ws.numel(), nat.stream_ptr())
        nat.check(rc)
        return out_ids, out_scores

    # ------------------------------------------------------------------ hot path
    def search_device(self, q_dev, k: int, eta: float, entropy_pref: float, out_ids=None, out_scores=None,
                      candidates: Optional[int] = None, similarity: str = "ip", use_shadow: bool = True,
                      filter: Optional[DeviceFilter] = None):
        """Enqueue one search on the current stream; returns device tensors, no sync.

        q_dev: fp32 [B, d] on this device (raw queries; cosine normalisation happens in-kernel).
        ``candidates``: size of the similarity cut that is re-ranked; default min(2k, N) as the
        reference's ExactIndex, ``candidates=k`` gives the rule of its HNSW / FAISS backends, whose
        blend uses ``similarity`` = "ip" (faiss inner product, the raw score), "one_minus_dist"
        (hnswlib: 1 - dist) or "inv_one_plus_dist" (faiss L2: 1/(1+dist)) — reference
        backends.py:229-231, 335-338.

        NOT thread-safe on one instance (shared workspaces).  Always answered: a query that a matrix-core pass of
        the batch refuses (adversarial corpora) is repaired inside the library call, on the same stream (ABI 5) — no
        id -1 ever reaches the outputs, so there is nothing for the caller to check after synchronising.

        ``filter`` (a ``DeviceFilter`` of this corpus): search only its rows (ABI 6) — the fp32 row kernels over the
        list, whatever the batch size; ids stay rows of the whole corpus.  Results are [B, 0] when k <= 0 or the filter
        is empty.  A ``DeviceQueryFilters`` of B lists: query j searches only its own list (``_search_query_filtered``);
        the results keep their [B, k] shape and the row of a query whose list is empty holds id -1 and score NaN.
        """
        if isinstance(filter, DeviceQueryFilters):
            return self._search_query_filtered(q_dev, k, eta, entropy_pref, out_ids, out_scores, candidates, similarity,
                                               filter)
        if filter is not None:
            return self._search_filtered(q_dev, k, eta, entropy_pref, out_ids, out_scores, candidates, similarity, filter)
        n, d = self.n_rows, self.dim
        b, k = check_search_args(q_dev.shape, d, k, candidates, similarity)
        if k <= 0:
            return empty_result(b, self.device)
        c = cut_size(k, candidates, n)
        if out_ids is None or out_scores is None:
            out_ids, out_scores = default_outputs(b, k, self.device, out_ids, out_scores)
        # (the cache directly, with the shape read once: the hit path of the headline step)
        ws = self._cached_workspace((b, c), self._lib.dewi_knn_workspace_bytes, n, d, b, c)
        through_shadow = candidates is None and self.shadow is not None and b >= self.shadow_min_batch and use_shadow
        self._last_call = (b, k, c, bool(through_shadow), ws)
        if through_shadow:
            rc = self._lib.dewi_knn_rerank_f32_shadow(
                nat.ptr(self.emb), nat.ptr(self.shadow), self.n_rows, self.dim, nat.ptr(q_dev), b, nat.ptr(self.dewi32),
                nat.ptr(self.ent32), k, float(eta), float(entropy_pref), nat.SPACE_CODES[self.space], nat.ptr(out_ids),
                nat.ptr(out_scores), nat.ptr(ws), ws.numel(), nat.stream_ptr())
        elif candidates is None:
            fn = self._lib.dewi_knn_rerank_bf16 if self.is_bf16 else self._lib.dewi_knn_rerank_f32
            rc = fn(nat.ptr(self.emb), self.n_rows, self.dim, nat.ptr(q_dev), b, nat.ptr(self.dewi32),
                    nat.ptr(self.ent32), k, float(eta), float(entropy_pref), nat.SPACE_CODES[self.space],
                    nat.ptr(out_ids), nat.ptr(out_scores), nat.ptr(ws), ws.numel(), nat.stream_ptr())
        else:
            rc = self._lib.dewi_knn_rerank_candidates(
                nat.ptr(self.emb), self._elem, self.n_rows, self.dim, nat.ptr(q_dev), b, nat.ptr(self.dewi32),
                nat.ptr(self.ent32), k, int(candidates), float(eta), float(entropy_pref), nat.SPACE_CODES[self.space],
                nat.SIM_CODES[similarity], nat.ptr(out_ids), nat.ptr(out_scores), nat.ptr(ws), ws.numel(), nat.stream_ptr())
        nat.check(rc)
        return out_ids, out_scores

    # ------------------------------------------------------------------ range search
    def stage_thresholds(self, thresholds, n_queries: int):
        """A scalar or [B] thresholds (numbers, numpy or torch) -> fp32 [B] tensor on this device.  The length is checked
        before anything touches the device."""
        torch = _torch()
        if isinstance(thresholds, torch.Tensor):
            t = thresholds.reshape(-1) if thresholds.dim() == 0 else thresholds
            if t.dim() != 1 or int(t.shape[0]) not in (1, n_queries):
                raise ValueError(f"thresholds must be a scalar or have shape ({n_queries},), got {tuple(thresholds.shape)}")
            t = t.to(device=self.device, dtype=torch.float32)
            return (t.expand(n_queries) if int(t.shape[0]) != n_queries else t).contiguous()
        return torch.from_numpy(check_thresholds(thresholds, n_queries)).to(self.device)

    def range_search_device(self, q_dev, thresholds, eta: float, entropy_pref: float, filter: Optional[DeviceFilter] = None,
                            max_results: Optional[int] = None, sort: bool = True):
        """``range_search_routed`` with ``use_shadow=True``: the shadow route wherever it applies, the dense route elsewhere —
        the same answer, bit for bit, either way."""
        return self.range_search_routed(q_dev, thresholds, eta, entropy_pref, filter=filter, max_results=max_results, sort=sort)

    def range_search_routed(self, q_dev, thresholds, eta: float, entropy_pref: float, filter: Optional[DeviceFilter] = None,
                            max_results: Optional[int] = None, sort: bool = True, use_shadow: bool = True):
        """Every row at least as similar to the query as its threshold, however many that is: device tensors
        ``(lims int64 [B + 1], rows int64 [T], sims fp32 [T], scores fp32 [T])`` — query j's rows are
        ``rows[lims[j]:lims[j + 1]]`` (``id_offset`` added), ``sims`` their similarities, ``scores`` the adjusted scores.

        The rule is steps 1-2 of the search (``dewi_hip.h``), the test ``sim >= threshold`` instead of a cut, then the
        blend: a row's ``sims`` / ``scores`` are bit for bit what the one-query search gives it, and a NaN similarity
        never passes.  ``space="l2"``: the similarity is ``-||e - q||^2``, so a radius r is ``threshold = -r * r``.
        ``thresholds``: one number, or one per query.  ``sort=True`` orders every query's segment as the search orders its
        answers (adjusted score descending, ties to the higher similarity, then to the lower row); ``sort=False`` leaves
        ascending rows.  ``filter``: a ``DeviceFilter`` of this corpus (fp32 corpora): only its rows are scanned.
        ``max_results``: raise ``ValueError`` — before the rows of the offending chunk are collected — once the batch has
        more rows than that.

        Two routes with the same answer, bit for bit.  DENSE: chunks of up to 32 queries: ``dewi_knn_range_count`` (dense row
        scan + count), ONE host synchronisation to read the chunk's counts and size its outputs, ``dewi_knn_range_collect``.
        SHADOW (``use_shadow``, an fp32 corpus with ``enable_bf16_shadow``, no filter, a shape
        ``dewi_knn_range_shadow_supported`` takes, at least ``range_shadow_min_batch`` queries): chunks of up to 2048 queries,
        one pass over the bf16 copy per 256 of them, the same one synchronisation per chunk; a query whose survivor segment
        overflowed is answered by the dense route and spliced back.  The workspace belongs to the chunk between its two
        calls: NOT thread-safe on one instance."""
        lims, rows, sims, scores, ascending = self._range_rows(q_dev, thresholds, eta, entropy_pref, filter, max_results, use_shadow)
        torch = _torch()
        dev = self.device
        b = int(q_dev.shape[0])
        if rows.shape[0] == 0:
            return lims, rows, sims, scores
        # plumbing from here on (torch): the order inside a query's segment
        seg = None
        if b > 1 and (sort or not ascending):  # the query of every result, as the high bits of a sort key
            seg = torch.bucketize(torch.arange(rows.shape[0], dtype=torch.int64, device=dev), lims[1:], right=True)
        if not ascending:
            # a filter over rows that are not whole 16-byte units is scanned bucket by bucket, and the shadow route leaves
            # the order of its survivor segments: ascending rows first
            order = torch.argsort(rows if seg is None else seg * (1 << 32) + rows, stable=True)
            rows, sims, scores = rows[order], sims[order], scores[order]
        if sort:
            # two stable sorts over ascending rows: by similarity, then by (query, adjusted score) — ties on the adjusted
            # score keep the higher similarity first, ties on both the lower row
            o1 = torch.sort(-_order_key(sims), stable=True).indices
            key = (1 << 32) - _order_key(scores[o1])
            o2 = torch.sort(key if seg is None else seg[o1] * (1 << 34) + key, stable=True).indices
            order = o1[o2]
            rows, sims, scores = rows[order], sims[order], scores[order]
        if self.id_offset:
            rows = rows + self.id_offset
        return lims, rows, sims, scores

    def _range_rows(self, q_dev, thresholds, eta: float, entropy_pref: float, filter, max_results, use_shadow: bool,
                    first_row: int = 0):
        """The two routes of ``range_search_device``: ``(lims, LOCAL rows, sims, scores, ascending)`` in query order;
        ``ascending``: every query's rows already ascend.  ``first_row`` (the self-join): rows below it are not wanted — the
        shadow route does not scan them, the dense route returns them all the same."""
        torch = _torch()
        if isinstance(filter, DeviceQueryFilters):
            raise NotImplementedError("range search takes one allow-list for the batch (per-query filters: not in this build)")
        if filter is not None:
            self.check_filter(filter)
        b = int(q_dev.shape[0])
        if q_dev.dim() != 2 or q_dev.shape[1] != self.dim:
            raise ValueError(f"Expected query shape ({self.dim},), got {tuple(q_dev.shape[1:])}")
        thr = self.stage_thresholds(thresholds, b)
        if filter is not None and self.is_bf16:
            raise NotImplementedError("filtered search serves fp32 corpora (bf16: not in this build)")
        dev = self.device
        through_shadow = (use_shadow and self.shadow is not None and filter is None and not self.is_bf16
                          and b >= max(1, int(self.range_shadow_min_batch))
                          and bool(self._lib.dewi_knn_range_shadow_supported(self.n_rows, self.dim, nat.SPACE_CODES[self.space])))
        budget = _RangeBudget(max_results, b)
        if through_shadow:
            counts_h, parts = self._range_shadow(q_dev, thr, eta, entropy_pref, budget, int(first_row))
            lims_c = None
        else:
            counts_h, parts, lims_c = self._range_dense(q_dev, thr, eta, entropy_pref, filter, budget)
        if lims_c is not None and b <= nat.RANGE_MAX_QUERIES and parts:
            lims = lims_c                      # one chunk: its running sum is the batch's
        else:
            lims_h = np.zeros(b + 1, dtype=np.int64)
            np.cumsum(counts_h, out=lims_h[1:])
            lims = torch.from_numpy(lims_h).to(dev)
        if not parts:
            return (lims, torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                    torch.empty(0, dtype=torch.float32, device=dev), True)
        rows, sims, scores = parts[0] if len(parts) == 1 else tuple(torch.cat(x) for x in zip(*parts))
        ascending = not through_shadow and not (filter is not None and self.dim % 4 != 0)
        return lims, rows, sims, scores, ascending

    def _range_dense(self, q_dev, thr, eta: float, entropy_pref: float, filter, budget: "_RangeBudget"):
        """The dense route over all of ``q_dev``: ``(counts int64 [B] on the host, [(rows, sims, scores)] per chunk with
        rows, the last chunk's device lims)``."""
        torch = _torch()
        b = int(q_dev.shape[0])
        n_scan = self.n_rows if filter is None else filter.n_allowed
        dev = self.device
        parts = []
        counts_h = np.zeros(b, dtype=np.int64)
        elem = self._elem
        lims_c = None
        for q0 in range(0, b if n_scan > 0 else 0, nat.RANGE_MAX_QUERIES):
            nb = min(nat.RANGE_MAX_QUERIES, b - q0)
            ws = self._cached_workspace(("range", nb, n_scan), self._lib.dewi_knn_range_workspace_bytes, n_scan, self.dim, elem, nb)
            q_c, thr_c = q_dev[q0:q0 + nb], thr[q0:q0 + nb]
            counts_d = torch.empty(nb, dtype=torch.int64, device=dev)
            nat.check(self._lib.dewi_knn_range_count(
                nat.ptr(self.emb), elem, self.n_rows, self.dim, nat.ptr(filter.buf) if filter is not None else None,
                n_scan if filter is not None else 0, nat.ptr(q_c), nb, nat.ptr(thr_c), nat.SPACE_CODES[self.space],
                nat.ptr(counts_d), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
            c_h = counts_d.cpu().numpy()                   # the chunk's one synchronisation
            counts_h[q0:q0 + nb] = c_h
            t_c = int(c_h.sum())
            budget.add(t_c, nb)
            if t_c == 0:
                continue
            lims_c = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts_d, 0, out=lims_c[1:])
            rows = torch.empty(t_c, dtype=torch.int64, device=dev)
            sims = torch.empty(t_c, dtype=torch.float32, device=dev)
            scores = torch.empty(t_c, dtype=torch.float32, device=dev)
            nat.check(self._lib.dewi_knn_range_collect(
                nat.ptr(ws), ws.numel(), n_scan, nb, nat.ptr(thr_c), nat.ptr(lims_c), t_c, nat.ptr(self.dewi32),
                nat.ptr(self.ent32), float(eta), float(entropy_pref), nat.ptr(rows), nat.ptr(sims), nat.ptr(scores),
                nat.stream_ptr()))
            parts.append((rows, sims, scores))
        return counts_h, parts, lims_c

    def _range_shadow(self, q_dev, thr, eta: float, entropy_pref: float, budget: "_RangeBudget", first_row: int):
        """The shadow route over all of ``q_dev`` (rows from ``first_row`` on): ``(counts int64 [B] on the host, [(rows, sims,
        scores)] per chunk)``, every query's rows in the order of its survivor segments (a repaired query's: ascending)."""
        torch = _torch()
        b = int(q_dev.shape[0])
        dev = self.device
        seg_cap = int(self.range_shadow_seg_cap)
        parts = []
        counts_h = np.zeros(b, dtype=np.int64)
        for q0 in range(0, b, nat.RANGE_SHADOW_MAX_QUERIES):
            nb = min(nat.RANGE_SHADOW_MAX_QUERIES, b - q0)
            ws = self._cached_workspace(("range_shadow", nb, seg_cap), self._lib.dewi_knn_range_shadow_workspace_bytes,
                                        self.n_rows, self.dim, nat.SPACE_CODES[self.space], nb, seg_cap)
            q_c, thr_c = q_dev[q0:q0 + nb], thr[q0:q0 + nb]
            counts_d = torch.empty(nb, dtype=torch.int64, device=dev)
            nat.check(self._lib.dewi_knn_range_shadow_count(
                nat.ptr(self.emb), nat.ptr(self.shadow), self.n_rows, self.dim, first_row, nat.ptr(q_c), nb, nat.ptr(thr_c),
                seg_cap, nat.ptr(counts_d), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
            c_h = counts_d.cpu().numpy()                   # the chunk's one synchronisation
            flagged = np.flatnonzero(c_h < 0)
            c_ok = np.where(c_h < 0, 0, c_h)
            t_c = int(c_ok.sum())
            budget.add(t_c, nb - int(flagged.size))     # (the flagged queries are counted by their dense repair)
            lims_ok = np.zeros(nb + 1, dtype=np.int64)
            np.cumsum(c_ok, out=lims_ok[1:])
            rows = torch.empty(t_c, dtype=torch.int64, device=dev)
            sims = torch.empty(t_c, dtype=torch.float32, device=dev)
            scores = torch.empty(t_c, dtype=torch.float32, device=dev)
            if t_c:
                lims_c = torch.from_numpy(lims_ok).to(dev)
                nat.check(self._lib.dewi_knn_range_shadow_collect(
                    nat.ptr(ws), ws.numel(), self.n_rows, self.dim, first_row, nb, seg_cap, nat.ptr(lims_c), t_c,
                    nat.ptr(self.dewi32), nat.ptr(self.ent32), float(eta), float(entropy_pref), nat.ptr(rows), nat.ptr(sims),
                    nat.ptr(scores), nat.stream_ptr()))
            if flagged.size:
                # overflowed queries: the dense route, gathered into dense chunks of <= 32, spliced back into their places
                idx = torch.from_numpy(flagged).to(dev)
                d_counts, d_parts, _ = self._range_dense(q_c[idx].contiguous(), thr_c[idx].contiguous(), eta, entropy_pref, None,
                                                         budget)
                d_lims = np.zeros(flagged.size + 1, dtype=np.int64)
                np.cumsum(d_counts, out=d_lims[1:])
                c_fin = c_ok.copy()
                c_fin[flagged] = d_counts
                starts = lims_ok[:-1].copy()               # where each query's rows start in [shadow rows | dense rows]
                starts[flagged] = t_c + d_lims[:-1]
                out_lims = np.zeros(nb + 1, dtype=np.int64)
                np.cumsum(c_fin, out=out_lims[1:])
                gather = np.repeat(starts - out_lims[:-1], c_fin) + np.arange(int(out_lims[-1]), dtype=np.int64)
                g = torch.from_numpy(gather).to(dev)
                both = [torch.cat([x] + [p[i] for p in d_parts]) for i, x in enumerate((rows, sims, scores))]
                rows, sims, scores = both[0][g], both[1][g], both[2][g]
                c_ok = c_fin
            counts_h[q0:q0 + nb] = c_ok
            if rows.shape[0]:
                parts.append((rows, sims, scores))
        return counts_h, parts

    # ------------------------------------------------------------------ near-duplicate self-join
    def near_duplicates_device(self, threshold: float, chunk: int = 2048, max_pairs: Optional[int] = None,
                               use_shadow: bool = True):
        """Every pair of stored rows at least ``threshold`` similar: device tensors ``(a int64 [P], b int64 [P], sims fp32
        [P])`` with ``a < b``, ordered by ``(a, b)`` (``id_offset`` added to both).

        DEFINITION: the pair ``(a, b)``, ``a < b``, is reported iff row ``b`` is in ``range_search(E[a], threshold)`` — the
        stored row ``a`` as the query — and ``sims`` is that directed similarity.  (Similarities are not bit-symmetric: the
        query side is normalised once more, so the direction is part of the contract.)

        The queries are slices of the stored matrix (no host copy), ``chunk`` rows (at most 2048) at a time; chunk ``[s, e)``
        scans only the rows from ``s`` on, which makes the join the upper triangle.  With a bf16 shadow every chunk is one
        ``range_search_routed`` batch on the shadow route; anything else (``use_shadow=False``, l2, bf16 corpora, other
        widths) runs the same definition on the dense route, slowly.  ``max_pairs``: ``ValueError`` once there are more pairs
        — before a chunk is collected when its counts alone prove it (they include each query's rows up to itself, at most
        ``chunk * (chunk + 1) / 2`` per chunk), otherwise right after it."""
        torch = _torch()
        dev = self.device
        n = self.n_rows
        chunk = max(1, min(int(chunk), nat.RANGE_SHADOW_MAX_QUERIES))
        thr = float(threshold)
        out = []
        pairs = 0
        for s in range(0, n - 1, chunk):
            e = min(n, s + chunk)
            nb = e - s
            q = self.emb[s:e] if not self.is_bf16 else self.emb[s:e].float()
            room = None if max_pairs is None else int(max_pairs) - pairs + nb * (nb + 1) // 2
            try:
                lims, rows, sims, _, ascending = self._range_rows(q, thr, 0.0, 0.0, None, room, use_shadow, first_row=s)
            except ValueError as err:
                if max_pairs is not None and "max_results" in str(err):
                    raise ValueError(f"near_duplicates found more than max_pairs = {int(max_pairs)} pairs (rows {s} to {e} of "
                                     f"{n}): raise the threshold or max_pairs") from None
                raise
            if rows.shape[0] == 0:
                continue
            a = torch.bucketize(torch.arange(rows.shape[0], dtype=torch.int64, device=dev), lims[1:], right=True) + s
            keep = rows > a
            a, rows, sims = a[keep], rows[keep], sims[keep]
            if not ascending:
                order = torch.argsort(a * (1 << 32) + rows, stable=True)
                a, rows, sims = a[order], rows[order], sims[order]
            pairs += int(a.shape[0])
            if max_pairs is not None and pairs > int(max_pairs):
                raise ValueError(f"near_duplicates found more than max_pairs = {int(max_pairs)} pairs (rows {s} to {e} of {n}): "
                                 f"raise the threshold or max_pairs")
            out.append((a, rows, sims))
        if not out:
            return (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                    torch.empty(0, dtype=torch.float32, device=dev))
        a, rows, sims = out[0] if len(out) == 1 else tuple(torch.cat(x) for x in zip(*out))
        if self.id_offset:
            a, rows = a + self.id_offset, rows + self.id_offset
        return a, rows, sims

    # ------------------------------------------------------------------ near-duplicate groups
    def _groups_begin(self, n: int):
        """A union-find over rows ``0 .. n - 1`` in this corpus's cached workspace, every row its own group."""
        if not 1 <= int(n) < (1 << 31):
            raise ValueError(f"groups need between 1 and 2^31 - 1 rows, got {n}")
        ws = self._cached_workspace(("groups", int(n)), self._lib.dewi_groups_workspace_bytes, int(n))
        nat.check(self._lib.dewi_groups_begin(int(n), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return ws

    def _groups_finish(self, ws, n: int, keep: str):
        """``((labels, sizes, representatives) int64 [n] on the device, n_groups)`` of the workspace's edges so far; the one
        synchronisation of a grouping.  Edges with an endpoint outside the rows: ``ValueError``."""
        torch = _torch()
        if keep not in nat.KEEP_CODES:
            raise ValueError(f"unknown keep rule {keep!r}: one of {sorted(nat.KEEP_CODES)}")
        if keep == "dewi" and int(n) != self.n_rows:
            raise ValueError(f"keep='dewi' reads this corpus's dewi column: {self.n_rows} rows, not {n}")
        labels, sizes, reps = (torch.empty(int(n), dtype=torch.int64, device=self.device) for _ in range(3))
        n_groups, bad = ctypes.c_int64(0), ctypes.c_int64(0)
        nat.check(self._lib.dewi_groups_finish(int(n), nat.KEEP_CODES[keep], nat.ptr(self.dewi32) if keep == "dewi" else None,
                                               self.id_offset, nat.ptr(labels), nat.ptr(sizes), nat.ptr(reps), ctypes.byref(n_groups),
                                               ctypes.byref(bad), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        if bad.value:
            raise ValueError(f"{bad.value} edges have an endpoint outside the {n} rows")
        return (labels, sizes, reps), int(n_groups.value)

    def duplicate_groups_device(self, threshold: float, chunk: int = 2048, use_shadow: bool = True, keep: str = "first"):
        """The near-duplicate GROUPS of the stored rows: ``((labels, sizes, representatives), n_groups)`` — three int64 [N]
        device tensors and the number of groups (singletons included).

        DEFINITION: the groups are the connected components of the graph whose edges are exactly the pairs
        ``near_duplicates_device(threshold)`` reports (single linkage: a chain of pairwise-similar rows is one group).
        ``labels[i]``: the smallest row of row i's group (``id_offset`` added) — the same whatever the chunking or the order
        the device took the edges in; ``sizes[i]``: the group's number of rows; ``representatives[i]``: the one row that stands
        for the group (``id_offset`` added) — ``keep="first"`` its smallest row, ``keep="dewi"`` the row with the highest
        ``dewi32`` (ties to the lower row; a NaN loses to every number).

        The chunk loop, the ``_range_rows`` call and the routes are those of ``near_duplicates_device``; every chunk's result
        lists go straight into ``dewi_groups_union_lists`` (which skips each query's own and lower rows) and are dropped: no
        pair is kept, so there is no ``max_pairs`` — memory is O(N) plus one chunk's results.  One synchronisation per chunk
        (the range search's) and one at the end.  The workspace is this corpus's: NOT thread-safe on one instance."""
        n = self.n_rows
        chunk = max(1, min(int(chunk), nat.RANGE_SHADOW_MAX_QUERIES))
        thr = float(threshold)
        if keep not in nat.KEEP_CODES:
            raise ValueError(f"unknown keep rule {keep!r}: one of {sorted(nat.KEEP_CODES)}")
        ws = self._groups_begin(n)
        for s in range(0, n - 1, chunk):
            e = min(n, s + chunk)
            q = self.emb[s:e] if not self.is_bf16 else self.emb[s:e].float()
            lims, rows, _, _, _ = self._range_rows(q, thr, 0.0, 0.0, None, None, use_shadow, first_row=s)
            if rows.shape[0]:
                nat.check(self._lib.dewi_groups_union_lists(n, nat.ptr(lims), nat.ptr(rows), e - s, int(rows.shape[0]), s,
                                                            nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return self._groups_finish(ws, n, keep)

    def groups_from_pairs_device(self, a, b, n_rows: Optional[int] = None, keep: str = "first"):
        """``duplicate_groups_device``'s result for the caller's own edges: ``a``, ``b`` int64 [P] device tensors of row ids as
        ``near_duplicates_device`` returns them (``id_offset`` included), in any order, repeats and ``a == b`` allowed.
        ``n_rows`` (default: this corpus's): the ids' range; ``keep="dewi"`` needs the corpus's own.  An id outside the
        range: ``ValueError``."""
        torch = _torch()
        n = self.n_rows if n_rows is None else int(n_rows)
        if keep not in nat.KEEP_CODES:
            raise ValueError(f"unknown keep rule {keep!r}: one of {sorted(nat.KEEP_CODES)}")
        a, b = (torch.as_tensor(x, dtype=torch.int64, device=self.device).reshape(-1).contiguous() for x in (a, b))
        if a.shape != b.shape:
            raise ValueError(f"a and b must have the same length, got {tuple(a.shape)} and {tuple(b.shape)}")
        if self.id_offset:
            a, b = a - self.id_offset, b - self.id_offset
        ws = self._groups_begin(n)
        nat.check(self._lib.dewi_groups_union_pairs(n, nat.ptr(a), nat.ptr(b), int(a.shape[0]), nat.ptr(ws), ws.numel(),
                                                    nat.stream_ptr()))
        return self._groups_finish(ws, n, keep)

    def refused_by_last_call(self) -> np.ndarray:
        """Monitoring / tests: bool [B] — which queries of the LAST ``search_device`` call a matrix-core pass refused (and the
        repair launches inside the same library call answered).  All False for a shape that takes the row kernels.
        Synchronises the current stream."""
        torch = _torch()
        b, k, c, through_shadow, ws = self._last_call
        off = ctypes.c_size_t(0)
        with torch.cuda.device(self.device):
            nat.check(self._lib.dewi_knn_refusal_flags(self._elem, 1 if through_shadow else 0, self.n_rows, self.dim,
                                                       b, k, c, nat.SPACE_CODES[self.space], ctypes.byref(off)))
            torch.cuda.current_stream().synchronize()
        if off.value == ctypes.c_size_t(-1).value:
            return np.zeros(b, dtype=bool)
        return ws[off.value: off.value + 4 * b].view(torch.int32).cpu().numpy() != 0

    def scan_kernel_name(self, n_queries: int, k: int, candidates: Optional[int] = None) -> str:
        """The kernel that streams the corpus for a batch of this size (``dewi_knn_scan_kernel``): measurement label."""
        c = cut_size(k, candidates, self.n_rows)
        buf = ctypes.create_string_buffer(128)
        with _torch().cuda.device(self.device):
            nat.check(self._lib.dewi_knn_scan_kernel(self._elem, self.n_rows, self.dim, int(n_queries), c,
                                                     nat.SPACE_CODES[self.space], buf, 128))
        return buf.value.decode()

    def search(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
               candidates: Optional[int] = None, similarity: str = "ip",
               filter: Optional[DeviceFilter] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking convenience: (ids int64 [B,k] including id_offset, scores fp32 [B,k]) on the host.
        Safe to call from several threads on one instance (serialised by a per-corpus lock).
        ``filter``: see ``search_device`` (an empty filter gives [B, 0]; per-query filters pad the row of a query with an
        empty list with id -1 and score NaN)."""
        torch = _torch()
        if isinstance(filter, DeviceQueryFilters):
            with self._lock, torch.cuda.device(self.device):
                q = self.stage_queries(queries)
                ids_d, sc_d = self.search_device(q, k, eta, entropy_pref, candidates=candidates, similarity=similarity,
                                                 filter=filter)
                ids_h, scores_h = ids_d.cpu().numpy(), sc_d.cpu().numpy()
            if self.id_offset:
                ids_h = np.where(ids_h >= 0, ids_h + self.id_offset, ids_h)
            return ids_h, scores_h
        if filter is not None:
            self.check_filter(filter)
            if filter.n_allowed == 0:
                k = 0
        with self._lock, torch.cuda.device(self.device):
            q = self.stage_queries(queries)
            # Small result sets (one query, a handful: what the reference's search returns) are written by the select kernel
            # STRAIGHT INTO pinned host memory (device-visible at its own address on ROCm; 12 bytes per result over PCIe): no
            # device buffer, no copy command, ONE stream synchronisation — 3.5 us less per blocking call than a device
            # buffer + async D2H copy (round 4: C1 45.4 -> 41.9 us p50, C2 464.0 -> 460.5).  Large batches keep the device
            # buffer and one DMA copy (tens of thousands of 4- and 8-byte stores over PCIe would cost more than they save).
            b, kk = int(q.shape[0]), max(int(k), 0)
            io = self._io.get((b, kk))
            if io is None:
                if len(self._io) > 8:
                    self._io.clear()
                # ids (int64) and scores (fp32) share one allocation, so that they return in one copy
                n_el = b * kk
                hbuf = torch.empty(n_el * 12, dtype=torch.uint8, pin_memory=True)
                dbuf = None if n_el <= 4096 else torch.empty(n_el * 12, dtype=torch.uint8, device=self.device)
                tgt = hbuf if dbuf is None else dbuf
                io = (tgt[: n_el * 8].view(torch.int64).view(b, kk), tgt[n_el * 8:].view(torch.float32).view(b, kk),
                      hbuf[: n_el * 8].view(torch.int64).view(b, kk), hbuf[n_el * 8:].view(torch.float32).view(b, kk),
                      dbuf, hbuf)
                self._io[(b, kk)] = io
            if kk > 0:
                self.search_device(q, k, eta, entropy_pref, io[0], io[1], candidates=candidates, similarity=similarity,
                                   filter=filter)
                if io[4] is not None:
                    io[5].copy_(io[4], non_blocking=True)
                torch.cuda.current_stream().synchronize()
            ids_h = io[2].numpy().copy()
            scores_h = io[3].numpy().copy()
            # (a query a matrix-core pass refused was repaired inside the library call, on the stream: ABI 5)
        if self.id_offset:
            ids_h = ids_h + self.id_offset
        return ids_h, scores_h

    def candidates_device(self, q_dev, n_candidates: int, out=None):
        """Per-shard top-``n_candidates`` records, int32 view [B, n_candidates, 4] (16 B each)."""
        b = int(q_dev.shape[0])
        out = self._records_out(b, n_candidates, out)
        c_local = max(1, min(n_candidates, self.n_rows))
        ws = self._workspace(b, c_local)
        self._last_call = (b, max(1, c_local // 2), c_local, False, ws)
        rc = self._lib.dewi_knn_candidates(nat.ptr(self.emb), self._elem, self.n_rows, self.dim,
                                           nat.ptr(q_dev), b, nat.ptr(self.dewi32), nat.ptr(self.ent32),
                                           int(n_candidates), nat.SPACE_CODES[self.space], self.id_offset, nat.ptr(out),
                                           nat.ptr(ws), ws.numel(), nat.stream_ptr())
        nat.check(rc)
        return out

    # ------------------------------------------------------------------ diverse search (MMR)
    def search_diverse_device(self, q_dev, k: int, eta: float, entropy_pref: float, mmr_lambda: float = 0.5,
                              candidates: Optional[int] = None, max_sim: Optional[float] = None, out_ids=None,
                              out_scores=None):
        """Enqueue one DIVERSE search on the current stream; returns device tensors ``(ids, scores)`` [B, k], no sync.

        The pool is the search's own candidate cut — ``candidates_device``: the ``candidates`` most similar rows of every
        query (default ``4k``, at most N and ``DIVERSE_MAX_CANDIDATES``) — and ``dewi_diverse_rerank`` picks from it
        greedily by maximal marginal relevance: ``mmr_lambda * adjusted score - (1 - mmr_lambda) * (largest inner product
        with a row already picked)``; a candidate at least ``max_sim`` similar to a picked row is struck out (``None``: no
        such cut).  Results are in PICK order; ``scores`` are the adjusted scores ``search_device`` returns.  ``mmr_lambda =
        1`` without ``max_sim`` is the plain search over that pool.  A query with fewer than k eligible rows leaves id -1 /
        score NaN in the tail of its row.  Cosine corpora (``space="l2"``: ``NotImplementedError`` — the
        penalty is an inner product of unit rows), fp32 and bf16.  NOT thread-safe on one instance (shared workspaces)."""
        return self._search_diverse(q_dev, k, eta, entropy_pref, mmr_lambda, candidates, max_sim, out_ids, out_scores)

    def search_diverse_approx_device(self, q_dev, k: int, eta: float, entropy_pref: float, mmr_lambda: float = 0.5,
                                     candidates: Optional[int] = None, max_sim: Optional[float] = None, rescore: bool = True,
                                     out_ids=None, out_scores=None):
        """``search_diverse_device`` with the pool taken by the int8 scores of the shadow (``candidates_i8_device``) and —
        ``rescore=True`` — re-scored from the fp32 rows; the same records then go to ``dewi_diverse_rerank`` with the fp32
        rows.  (A method of its own: the parameter list of ``search_diverse_device`` is fixed.)"""
        self._int8()
        return self._search_diverse(q_dev, k, eta, entropy_pref, mmr_lambda, candidates, max_sim, out_ids, out_scores,
                                    approx=True, rescore=rescore)

    def _search_diverse(self, q_dev, k, eta, entropy_pref, mmr_lambda, candidates, max_sim, out_ids, out_scores,
                        approx: bool = False, rescore: bool = True):
        torch = _torch()
        n = self.n_rows
        b, k = check_search_args(q_dev.shape, self.dim, k, None, "ip")
        if self.space == "l2":
            raise NotImplementedError("diverse search penalises the inner product of unit rows: space='l2' is not in this build")
        lam = float(mmr_lambda)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"mmr_lambda must lie in [0, 1], got {mmr_lambda}")
        cut = float("inf") if max_sim is None else float(max_sim)
        if cut != cut:
            raise ValueError("max_sim must not be NaN")
        if candidates is not None and int(candidates) > nat.DIVERSE_MAX_CANDIDATES:
            raise NotImplementedError(f"diverse search takes pools of at most {nat.DIVERSE_MAX_CANDIDATES} candidates, "
                                      f"got {int(candidates)}")
        if k <= 0:
            return empty_result(b, self.device)
        c = min(cut_size(k, 4 * k if candidates is None else int(candidates), n), nat.DIVERSE_MAX_CANDIDATES)
        if k > c:
            raise ValueError(f"k = {k} exceeds the pool of {c} candidates")
        out_ids, out_scores = default_outputs(b, k, self.device, out_ids, out_scores)
        if max_sim is not None:         # (without the cut every query picks k of its c >= k records: nothing is left unwritten)
            out_ids.fill_(-1)
            out_scores.fill_(float("nan"))
        if approx:
            recs = self.candidates_i8_device(q_dev, c)
            if rescore:
                self.rescore_candidates_device(q_dev, recs)
        else:
            recs = self.candidates_device(q_dev, c)
        need = int(self._lib.dewi_diverse_workspace_bytes(b, c, self.dim))    # 0: the re-rank keeps its state on chip
        ws = None
        if need:
            ws = self._cached_workspace(("diverse", b, c), self._lib.dewi_diverse_workspace_bytes, b, c, self.dim)
        rc = self._lib.dewi_diverse_rerank(
            nat.ptr(self.emb), self._elem, n, self.dim, nat.ptr(recs), b, c, k, float(eta), float(entropy_pref), lam, cut,
            self.id_offset, nat.ptr(out_ids), nat.ptr(out_scores), None, nat.ptr(ws) if ws is not None else None,
            ws.numel() if ws is not None else 0, nat.stream_ptr())
        nat.check(rc)
        return out_ids, out_scores

    def search_diverse(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                       mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                       max_sim: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking twin of ``search`` for ``search_diverse_device``: (ids int64 [B, k] — global, as the candidate records
        carry them —, scores fp32 [B, k]) on the host, in pick order; the tail of a short row holds id -1 / score NaN.  Safe to
        call from several threads on one instance (serialised by the per-corpus lock)."""
        return self._blocking(self.search_diverse_device, queries, k, eta, entropy_pref, mmr_lambda, candidates, max_sim, ids="global")

    def search_diverse_approx(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                              mmr_lambda: float = 0.5, candidates: Optional[int] = None, max_sim: Optional[float] = None,
                              rescore: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """Blocking twin of ``search_diverse`` for ``search_diverse_approx_device``."""
        return self._blocking(self.search_diverse_approx_device, queries, k, eta, entropy_pref, mmr_lambda, candidates, max_sim,
                              rescore, ids="global")

    # ------------------------------------------------------------------ subset selection (greedy coverage of the whole corpus)
    def select_subset_device(self, budget: int, mmr_lambda: float = 0.5, max_sim: Optional[float] = None, relevance=None,
                             mask=None, seeds=None, return_coverage: bool = False, picks_per_pass: Optional[int] = None,
                             return_stats: bool = False, *, group_labels=None, n_groups: int = 0, per_group: int = 1,
                             group_quota=None, return_group_counts: bool = False):
        """Enqueue one SUBSET SELECTION on the current stream: the ``budget`` most informative rows that do not repeat each
        other (``dewi_select_begin`` / ``_seed`` / ``_run``, include/dewi_hip.h).  Greedy maximal marginal relevance over
        ALL rows: each pick is the row with the largest ``mmr_lambda * relevance - (1 - mmr_lambda) * (largest inner product
        with a row already picked)``; a row at least ``max_sim`` similar to a picked row is struck out (``None``: no such
        cut).  One pass over the rows still in play per pick.

        ``relevance``: fp32 [N] on this device (default: the ``dewi32`` column; a NaN entry makes its row unpickable);
        ``mask``: bool / uint8 [N] on this device, 0 = not pickable; ``seeds``: LOCAL rows (a sequence or an int64 device
        tensor) applied as picks before the first choice — they penalise, are not returned and do not count.

        Returns device tensors, no host synchronisation: ``(rows int64 [min(budget, N)] — global, prefilled with -1 —,
        gain fp32 — the marginal value at the pick, prefilled with NaN —, n_picked int64 [1])``, in pick order; with
        ``return_coverage`` also ``(pen fp32 [N], owner int64 [N])``: every row's largest similarity to the selection (NaN:
        none; frozen once the row was struck out) and the global row that gave it (-1: none).  Cosine / inner-product rows
        (``space="l2"``: ``NotImplementedError``), fp32 and bf16.  NOT thread-safe on one instance (shared workspace).

        ``picks_per_pass``: ``None`` or 1 is the form above.  An integer above 1 takes the BLOCKED form (``dewi_select_seed_blocked``
        / ``dewi_select_run_blocked``): the same selection bit for bit, with up to that many picks (clipped to
        ``dewi_select_block_max`` of the row shape; 0 there: the one-pick form) applied by one corpus pass.  It enqueues about
        ``1.25 * budget / block + 2`` rounds, reads the run's counters back and repeats with the remaining budget until the
        run is finished: ONE HOST SYNCHRONISATION PER CHUNK, unlike the one-pick form.  ``return_stats`` appends a dict
        ``{"rounds", "passes", "picks_per_pass"}`` to the result (one-pick form: one round and one pass per pick).

        ``group_labels`` (keyword-only, with the arguments behind it): GROUP QUOTAS — at most ``per_group`` picks from one
        group (``dewi_select_groups_begin`` / ``dewi_select_run_grouped`` / ``dewi_select_run_blocked_grouped``).  An int32
        tensor [N] on this device, DENSE: row i is grouped when ``0 <= label < n_groups``, anything else is free of any quota
        (``dense_group_labels`` makes such labels).  ``group_quota``: an int32 tensor [n_groups] on this device, one quota per
        group, instead of ``per_group`` (<= 0: nothing is picked from that group).  Seeds do not count against a quota.
        ``return_group_counts`` appends the picks made per group (int32 [n_groups], behind the coverage, before the stats)."""
        torch = _torch()
        n = self.n_rows
        if self.space == "l2":
            raise NotImplementedError("subset selection penalises the inner product of unit rows: space='l2' is not in this build")
        lam = float(mmr_lambda)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"mmr_lambda must lie in [0, 1], got {mmr_lambda}")
        cut = float("inf") if max_sim is None else float(max_sim)
        if cut != cut:
            raise ValueError("max_sim must not be NaN")
        b = min(int(budget), n)
        if b < 0:
            raise ValueError(f"budget must not be negative, got {budget}")
        if return_coverage and b == 0:
            raise ValueError("return_coverage needs a budget of at least 1 (a run of no picks writes nothing)")
        rel = self.dewi32 if relevance is None else relevance
        if tuple(rel.shape) != (n,) or rel.dtype != torch.float32 or rel.device != self.device:
            raise ValueError(f"relevance must be a float32 tensor of shape ({n},) on {self.device}")
        rel = rel.contiguous()
        m8 = None
        if mask is not None:
            if tuple(mask.shape) != (n,) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != self.device:
                raise ValueError(f"mask must be a bool or uint8 tensor of shape ({n},) on {self.device}")
            m8 = mask.contiguous().view(torch.uint8)
        seed_rows = None
        if seeds is not None:
            seed_rows = (seeds if isinstance(seeds, torch.Tensor) else torch.as_tensor(np.asarray(seeds, np.int64).reshape(-1)))
            seed_rows = seed_rows.to(device=self.device, dtype=torch.int64).contiguous()
        rows = torch.full((b,), -1, dtype=torch.int64, device=self.device)
        gain = torch.full((b,), float("nan"), dtype=torch.float32, device=self.device)
        n_picked = torch.zeros(1, dtype=torch.int64, device=self.device)
        pen = owner = None
        if return_coverage:
            pen = torch.empty(n, dtype=torch.float32, device=self.device)
            owner = torch.empty(n, dtype=torch.int64, device=self.device)
        block = 1
        if picks_per_pass is not None:
            block = int(picks_per_pass)
            if block < 1:
                raise ValueError(f"picks_per_pass must be at least 1, got {picks_per_pass}")
            if block > 1:
                block = min(block, int(self._lib.dewi_select_block_max(self.dim, self._elem))) or 1
        stream = nat.stream_ptr()
        grp, counts = (), None
        if group_labels is not None:
            g = int(n_groups)
            if g < 1:
                raise ValueError(f"n_groups must be at least 1, got {n_groups}")
            if tuple(group_labels.shape) != (n,) or group_labels.dtype != torch.int32 or group_labels.device != self.device:
                raise ValueError(f"group_labels must be an int32 tensor of shape ({n},) on {self.device}")
            if group_quota is None and int(per_group) < 1:
                raise ValueError(f"per_group must be at least 1, got {per_group}")
            if group_quota is not None and (tuple(group_quota.shape) != (g,) or group_quota.dtype != torch.int32
                                            or group_quota.device != self.device):
                raise ValueError(f"group_quota must be an int32 tensor of shape ({g},) on {self.device}")
            lab = group_labels.contiguous()
            quota = None if group_quota is None else group_quota.contiguous()
            counts = torch.zeros(g, dtype=torch.int32, device=self.device)
            grp = (nat.ptr(lab), g, nat.ptr(quota) if quota is not None else None, int(per_group) if quota is None else 1,
                   nat.ptr(counts))
        elif return_group_counts:
            raise ValueError("return_group_counts needs group_labels")

        def workspace(size):
            # one workspace for every form: each layout is the one before it plus regions behind it, so an entry that a smaller
            # form sized is dropped here once and the larger one serves every later call of any form
            hit = self._ws.get(("select", n))
            if hit is not None and hit[0].numel() < library_size(*size):
                del self._ws[("select", n)]
            ws = self._cached_workspace(("select", n), *size)
            nat.check(self._lib.dewi_select_begin(n, self.dim, self._elem, nat.ptr(m8) if m8 is not None else None, nat.ptr(ws),
                                                  ws.numel(), stream))
            if grp:
                nat.check(self._lib.dewi_select_groups_begin(n, self.dim, self._elem, grp[1], nat.ptr(ws), ws.numel(), stream))
            return ws

        def finish(out, stats):
            out = out + ((pen, owner) if return_coverage else ()) + ((counts,) if return_group_counts else ())
            return out + (stats,) if return_stats else out

        if block > 1:
            if grp:
                ws = workspace((self._lib.dewi_select_grouped_workspace_bytes, n, self.dim, self._elem, grp[1], block))
            else:
                ws = workspace((self._lib.dewi_select_blocked_workspace_bytes, n, self.dim, self._elem, block))
            if seed_rows is not None and seed_rows.numel():
                nat.check(self._lib.dewi_select_seed_blocked(nat.ptr(self.emb), self._elem, n, self.dim, nat.ptr(seed_rows),
                                                             int(seed_rows.numel()), cut, nat.ptr(ws), ws.numel(), stream, block))
            stats_d = torch.zeros(3, dtype=torch.int64, device=self.device)
            rounds = passes = done = 0
            while done < b:
                left = b - done
                run = self._lib.dewi_select_run_blocked_grouped if grp else self._lib.dewi_select_run_blocked
                nat.check(run(
                    nat.ptr(self.emb), self._elem, n, self.dim, nat.ptr(rel), left, lam, cut, self.id_offset, nat.ptr(rows),
                    nat.ptr(gain), nat.ptr(n_picked), nat.ptr(pen) if pen is not None else None,
                    nat.ptr(owner) if owner is not None else None, nat.ptr(ws), ws.numel(), stream, block,
                    int(1.25 * left / block) + 2, nat.ptr(stats_d), *grp))
                st = stats_d.tolist()             # (the synchronisation of the chunk)
                rounds, passes = rounds + st[0], passes + st[1]
                if st[2]:
                    break
                done = int(n_picked.item())
            return finish((rows, gain, n_picked), {"rounds": rounds, "passes": passes, "picks_per_pass": block})
        if grp:
            ws = workspace((self._lib.dewi_select_grouped_workspace_bytes, n, self.dim, self._elem, grp[1], 0))
        else:
            ws = workspace((self._lib.dewi_select_workspace_bytes, n, self.dim, self._elem))
        if seed_rows is not None and seed_rows.numel():
            nat.check(self._lib.dewi_select_seed(nat.ptr(self.emb), self._elem, n, self.dim, nat.ptr(seed_rows),
                                                 int(seed_rows.numel()), cut, nat.ptr(ws), ws.numel(), stream))
        if b > 0:
            run = self._lib.dewi_select_run_grouped if grp else self._lib.dewi_select_run
            nat.check(run(
                nat.ptr(self.emb), self._elem, n, self.dim, nat.ptr(rel), b, lam, cut, self.id_offset, nat.ptr(rows),
                nat.ptr(gain), nat.ptr(n_picked), nat.ptr(pen) if pen is not None else None,
                nat.ptr(owner) if owner is not None else None, nat.ptr(ws), ws.numel(), stream, *grp))
        # (no read-back: the counters of the one-pick form are its launches)
        return finish((rows, gain, n_picked), {"rounds": b, "passes": b, "picks_per_pass": 1})

    # ------------------------------------------------------------------ collapsed search (at most m results per group)
    def make_groups(self, groups) -> DeviceGroups:
        """Prepare group labels for ``search_collapsed*``: whatever ``group_labels`` takes without an index — a
        ``DuplicateGroups``, an integer array [N] (negative: ungrouped) or a sequence of N hashables (``None``: ungrouped).
        The result is bound to the corpus as it stands (stale-checked like a ``DeviceFilter``)."""
        torch = _torch()
        lab, n_groups = group_labels(groups, self.n_rows)
        with torch.cuda.device(self.device):
            dev = torch.from_numpy(lab).to(self.device)
        return DeviceGroups(dev, n_groups, self.corpus_id, self.n_rows)

    def check_groups(self, groups: DeviceGroups) -> None:
        if not isinstance(groups, DeviceGroups):
            raise TypeError(f"expected DeviceGroups (make_groups), got {type(groups).__name__}")
        if groups.corpus_id != self.corpus_id:
            raise ValueError("these group labels were prepared for another corpus (the index was rebuilt or changed since): "
                             "prepare them again with make_groups")

    def candidates_filtered_device(self, q_dev, n_candidates: int, filter: DeviceFilter, out=None):
        """``candidates_device`` over the rows of ``filter`` only (``dewi_knn_candidates_filtered``; fp32 corpora, at most
        2048 records per query): int32 view [B, n_candidates, 4], ids rows of the whole corpus plus ``id_offset``, padding
        behind ``min(n_candidates, |A|)``.  An empty filter writes nothing: ``out`` is returned filled with padding."""
        self.check_filter(filter)
        b, c = int(q_dev.shape[0]), int(n_candidates)
        n_a = filter.n_allowed
        out = self._records_out(b, c, out, padded=n_a == 0)
        if n_a == 0:
            return out
        ws = self._cached_workspace(("filtered", b, n_a, min(c, n_a)), self._lib.dewi_knn_filtered_workspace_bytes, n_a, self.dim,
                                    b, c)
        nat.check(self._lib.dewi_knn_candidates_filtered(
            nat.ptr(self.emb), self._elem, self.n_rows, self.dim, nat.ptr(filter.buf), n_a, nat.ptr(q_dev), b,
            nat.ptr(self.dewi32), nat.ptr(self.ent32), c, nat.SPACE_CODES[self.space], self.id_offset, nat.ptr(out), nat.ptr(ws),
            ws.numel(), nat.stream_ptr()))
        return out

    # ------------------------------------------------------------------ search by examples
    def candidates_examples_device(self, x_dev, n_positive: int, n_candidates: int, *, match: str = "any",
                                   negative_rule: str = "penalty", negative_weight: float = 1.0, exclude=None,
                                   filter: Optional[DeviceFilter] = None, out=None):
        """The candidate cut of ONE request by examples (``dewi_knn_candidates_examples``): ``x_dev`` fp32 [P + N, d] raw
        example vectors on this device, the first ``n_positive`` of them positive.  Every row gets one combined score — the
        max (``match="any"``) or min (``"all"``) of its similarities to the positives, less ``negative_weight`` times its
        largest positive similarity to a negative (``negative_rule="penalty"``), or, with ``"best_score"``, minus that
        similarity squared where a negative is at least as near as the positives — and the ``n_candidates`` best rows
        come back as records, int32 view [1, n_candidates, 4], in ``candidates_device``'s layout and order; padding behind
        the rows offered.  ``exclude``: up to 16 LOCAL rows (int64 tensor on this device) that are never offered.  ``filter``:
        only the rows of one ``DeviceFilter`` are scanned; an empty one writes nothing: ``out`` is returned filled with
        padding.  fp32 cosine corpora of 132 to 4096 columns, ``dim % 4 == 0`` (``check_examples_shape``).  No sync."""
        check_examples_shape(self.space, self.is_bf16, self.dim)
        n_pos, n_neg = check_examples_request(int(n_positive), int(x_dev.shape[0]) - int(n_positive), match, negative_rule,
                                              negative_weight)
        if int(x_dev.shape[1]) != self.dim:
            raise ValueError(f"Expected examples of shape ({self.dim},), got {tuple(x_dev.shape[1:])}")
        c = int(n_candidates)
        if not 1 <= c <= EXAMPLES_MAX_CANDIDATES:
            raise ValueError(f"a search by examples re-ranks 1 to {EXAMPLES_MAX_CANDIDATES} candidates, got {c}")
        n_excl = 0 if exclude is None else int(exclude.shape[0])
        if n_excl > nat.EXAMPLES_MAX:
            raise ValueError(f"at most {nat.EXAMPLES_MAX} rows can be excluded, got {n_excl}")
        n_scan = self.n_rows
        if filter is not None:
            self.check_filter(filter)
            n_scan = filter.n_allowed
        empty = filter is not None and n_scan == 0
        out = self._records_out(1, c, out, padded=empty)
        if empty:
            return out
        ws = self._cached_workspace(("examples", n_scan, min(c, n_scan)), self._lib.dewi_knn_examples_workspace_bytes, n_scan,
                                    self.dim, n_pos + n_neg, c)
        nat.check(self._lib.dewi_knn_candidates_examples(
            nat.ptr(self.emb), self.n_rows, self.dim, nat.ptr(x_dev), n_pos, n_neg, nat.EXAMPLES_MATCH_CODES[match],
            nat.EXAMPLES_RULE_CODES[negative_rule], float(negative_weight), nat.ptr(exclude) if n_excl else None, n_excl,
            nat.ptr(filter.buf) if filter is not None else None, n_scan if filter is not None else 0, nat.ptr(self.dewi32),
            nat.ptr(self.ent32), c, self.id_offset, nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream_ptr()))
        return out

    def search_examples_device(self, x_dev, n_positive: int, k: int, eta: float, entropy_pref: float, *, match: str = "any",
                               negative_rule: str = "penalty", negative_weight: float = 1.0, candidates: Optional[int] = None,
                               exclude=None, filter: Optional[DeviceFilter] = None, n_offered: Optional[int] = None,
                               out_ids=None, out_scores=None):
        """Enqueue one search by examples on the current stream: ``candidates_examples_device`` for the cut —
        ``min(2k, rows offered)``, or ``candidates`` up to 2048 — then ``dewi_merge_rerank`` for the DEWI blend and the cut
        to k.  Returns device tensors ``(ids [1, k] as the records carry them, adjusted scores [1, k])``; [1, 0] for
        ``k <= 0`` or an empty filter; ``ValueError`` for k above the rows offered, as ``search`` raises it.
        ``n_offered``: the rows the request can return (scanned rows less the excluded rows among them) where the caller
        knows it; otherwise it is worked out here, which with both ``filter`` and ``exclude`` reads the filter's mask at the
        excluded rows (one small copy to the host)."""
        torch = _torch()
        check_examples_shape(self.space, self.is_bf16, self.dim)
        k = int(k)
        if filter is not None:
            self.check_filter(filter)
        n_scan = self.n_rows if filter is None else filter.n_allowed
        if k <= 0 or n_scan == 0:
            return empty_result(1, self.device)
        if n_offered is None:
            n_offered = n_scan
            if exclude is not None and int(exclude.shape[0]):
                rows = torch.unique(exclude)
                rows = rows[(rows >= 0) & (rows < self.n_rows)]
                n_offered -= int(rows.numel()) if filter is None else int(filter.byte_mask()[rows].ne(0).sum().item())
        n_offered = int(n_offered)
        if k > n_offered:
            raise ValueError(f"kth(={n_offered - k}) out of bounds ({n_offered})")
        if candidates is not None and int(candidates) < k:
            raise ValueError(f"n_candidates {int(candidates)} must be at least k = {k}")
        if candidates is not None and int(candidates) > EXAMPLES_MAX_CANDIDATES:
            raise ValueError(f"a search by examples re-ranks at most {EXAMPLES_MAX_CANDIDATES} candidates, got candidates = "
                             f"{int(candidates)}")
        c = cut_size(k, candidates, n_offered)
        if c > EXAMPLES_MAX_CANDIDATES:
            raise ValueError(f"a search by examples re-ranks at most {EXAMPLES_MAX_CANDIDATES} candidates, "
                             f"{'k = %d' % k if candidates is None else 'candidates = %d' % int(candidates)} asks for {c}")
        recs = self.candidates_examples_device(x_dev, n_positive, c, match=match, negative_rule=negative_rule,
                                               negative_weight=negative_weight, exclude=exclude, filter=filter)
        return merge_rerank_device(recs.unsqueeze(0), c, k, eta, entropy_pref, out_ids, out_scores)

    def collapse_rerank_device(self, recs, k: int, eta: float, entropy_pref: float, groups: DeviceGroups, per_group: int = 1,
                               out_ids=None, out_scores=None, out_hits=None, out_counts=None):
        """``dewi_collapse_rerank`` on candidate records of this corpus ([B, c, 4] int32 view, ids including ``id_offset``):
        ``(ids, scores, hits, counts)`` device tensors, no sync.  Outputs the caller does not pass are prefilled with
        -1 / NaN / 0 (positions from each query's count on are not written)."""
        torch = _torch()
        self.check_groups(groups)
        b, c = int(recs.shape[0]), int(recs.shape[1])
        if out_ids is None:
            out_ids = torch.full((b, k), -1, dtype=torch.int64, device=self.device)
        if out_scores is None:
            out_scores = torch.full((b, k), float("nan"), dtype=torch.float32, device=self.device)
        if out_hits is None:
            out_hits = torch.zeros((b, k), dtype=torch.int32, device=self.device)
        if out_counts is None:
            out_counts = torch.zeros(b, dtype=torch.int32, device=self.device)
        nat.check(self._lib.dewi_collapse_rerank(
            nat.ptr(recs), b, c, nat.ptr(groups.labels), self.n_rows, self.id_offset, int(k), int(per_group), float(eta),
            float(entropy_pref), nat.ptr(out_ids), nat.ptr(out_scores), nat.ptr(out_hits), nat.ptr(out_counts), None, 0,
            nat.stream_ptr()))
        return out_ids, out_scores, out_hits, out_counts

    def search_collapsed_device(self, q_dev, k: int, eta: float, entropy_pref: float, groups: DeviceGroups, per_group: int = 1,
                                candidates: Optional[int] = None, filter: Optional[DeviceFilter] = None, approx: bool = False,
                                rescore: bool = True, out_ids=None, out_scores=None, out_hits=None):
        """Enqueue one COLLAPSED search on the current stream: the k best documents of every query with at most ``per_group``
        of them from one group of ``groups`` (``make_groups``).  Returns device tensors ``(ids, scores, hits, counts)`` — ids
        [B, k] as the candidate records carry them (``id_offset`` included), adjusted scores, ``hits`` [B, k] the number of
        documents of the pool in the result's group (1 for an ungrouped one: what "+37 similar" shows) and ``counts`` [B] the
        number of results —, no sync.

        The pool is the search's own candidate cut: the ``candidates`` most similar rows of every query (default ``4k``, at
        most N — or the rows ``filter`` allows — and ``COLLAPSE_MAX_CANDIDATES`` = 2048), from ``candidates_device``, with
        ``filter`` (one ``DeviceFilter``; fp32 corpora) from ``candidates_filtered_device``, with ``approx=True`` (the int8
        shadow; pools up to 1024) from the int8 records, re-scored from the fp32 rows unless ``rescore=False``.
        ``dewi_collapse_rerank`` then walks the pool in the search's order and keeps a document unless ``per_group``
        documents of its group came before it.  The outputs are prefilled with -1 / NaN / 0: a query whose pool holds fewer
        than k groups' worth of documents has a short row.  Cosine and l2, fp32 and bf16 (no ``filter`` on bf16).  Per-query
        filters: ``NotImplementedError``.  ``k <= 0`` or an empty filter: [B, 0].  NOT thread-safe on one instance."""
        torch = _torch()
        self.check_groups(groups)
        if isinstance(filter, DeviceQueryFilters):
            raise NotImplementedError("a collapsed search takes one allow-list for the batch (per-query filters: not in this build)")
        if filter is not None:
            self.check_filter(filter)
            if self.is_bf16:
                raise NotImplementedError("filtered search serves fp32 corpora (bf16: not in this build)")
        b, k = check_search_args(q_dev.shape, self.dim, k, None, "ip")
        if int(per_group) <= 0:
            raise ValueError(f"per_group must be positive, got {per_group}")
        if approx:
            self._int8()
        n_avail = self.n_rows if filter is None else filter.n_allowed
        if k <= 0 or n_avail == 0:
            ids, sc = empty_result(b, self.device)
            return ids, sc, torch.zeros((b, 0), dtype=torch.int32, device=self.device), torch.zeros(b, dtype=torch.int32, device=self.device)
        c = collapse_pool(k, candidates, n_avail, approx)
        if k > c:
            raise ValueError(f"k = {k} exceeds the pool of {c} candidates")
        if approx:
            recs = self.candidates_i8_device(q_dev, c) if filter is None else self.candidates_i8_filtered_device(q_dev, c, filter)
            if rescore:
                self.rescore_candidates_device(q_dev, recs)
        elif filter is None:
            recs = self.candidates_device(q_dev, c)
        else:
            recs = self.candidates_filtered_device(q_dev, c, filter)
        if out_ids is not None:
            out_ids.fill_(-1)
        if out_scores is not None:
            out_scores.fill_(float("nan"))
        if out_hits is not None:
            out_hits.fill_(0)
        return self.collapse_rerank_device(recs, k, eta, entropy_pref, groups, per_group, out_ids, out_scores, out_hits)

    def search_collapsed(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, *, groups: DeviceGroups,
                         per_group: int = 1, candidates: Optional[int] = None, filter: Optional[DeviceFilter] = None,
                         approx: bool = False, rescore: bool = True, widen: bool = False, return_pool: bool = False):
        """Blocking twin of ``search_collapsed_device``: ``(ids int64 [B, k], scores fp32 [B, k], hits int32 [B, k])`` on the
        host — ids global, as the candidate records carry them; the tail of a short row holds -1 / NaN / 0.

        ``widen=True``: after a round each query's number of results is read back (one synchronisation per round); a query
        with fewer than k results whose pool was smaller than ``min(2048, N or |A|)`` is run again with four times the pool
        (capped there) and its row replaced, until no such query is left.  A query's final answer is by definition what
        ``search_collapsed(candidates=<its final pool>, widen=False)`` returns.  ``return_pool=True`` appends each query's
        final pool size (int64 [B]).  A query still short at the cap stays short (id -1): for groups larger than the cap,
        fold them corpus-wide with ``dedup_filter`` (or a filter of one row per group) instead.  Serialised by the per-corpus
        lock."""
        torch = _torch()
        with self._lock, torch.cuda.device(self.device):
            q = self.stage_queries(queries)
            ids_d, sc_d, hits_d, cnt_d = self.search_collapsed_device(q, k, eta, entropy_pref, groups, per_group, candidates, filter,
                                                                      approx, rescore)
            b, kk = int(ids_d.shape[0]), int(ids_d.shape[1])
            pool = np.zeros(b, dtype=np.int64)
            if kk > 0:
                n_avail = self.n_rows if filter is None else filter.n_allowed
                c = collapse_pool(kk, candidates, n_avail, approx)
                pool[:] = c
                limit = collapse_pool(kk, n_avail, n_avail, approx)          # the largest pool a round can take
                active = np.arange(b)
                while widen and c < limit:
                    counts = cnt_d.cpu().numpy()                            # the round's one synchronisation
                    active = active[counts < kk]
                    if active.size == 0:
                        break
                    c = min(4 * c, limit)
                    idx = torch.from_numpy(active).to(self.device)
                    out = self.search_collapsed_device(q[idx].contiguous(), kk, eta, entropy_pref, groups, per_group, c, filter,
                                                       approx, rescore)
                    ids_d[idx], sc_d[idx], hits_d[idx] = out[0], out[1], out[2]
                    cnt_d = out[3]
                    pool[active] = c
            res = (ids_d.cpu().numpy(), sc_d.cpu().numpy(), hits_d.cpu().numpy())
        return res + (pool,) if return_pool else res


class Int8Corpus(DeviceCorpus):
    """The int8 form of a corpus on its own (``DeviceCorpus.to_int8``): codes, scales and the two payload columns — no fp32
    rows.  Serves ``search_approx_device`` / ``search_approx`` with ``rescore=False``; every other public method of
    ``DeviceCorpus`` raises ``NotImplementedError``."""

    _SERVED = frozenset({"search_approx_device", "search_approx", "candidates_i8_device", "stage_queries", "corpus_bytes",
                         "cached_workspaces", "replace_cached_workspace", "drop_cached_workspaces"})

    def __init__(self, codes, scales, dewi32, ent32, id_offset: int = 0):
        torch = _torch()
        assert codes.is_cuda and codes.dim() == 2 and codes.is_contiguous() and codes.dtype == torch.int8
        assert scales.dtype == torch.float32 and int(scales.numel()) == int(codes.shape[0]) == int(dewi32.numel())
        self.emb = None
        self.i8_codes, self.i8_scales, self._i8_stale = codes, scales.contiguous(), False
        self.dewi32, self.ent32 = dewi32.contiguous(), ent32.contiguous()
        self.space = "cosine"
        self.id_offset = int(id_offset)
        self.device = codes.device
        self.corpus_id = next(_corpus_ids)
        self._lib = nat.load_library()
        self._ws = {}
        self._q_pinned = None
        self._q_dev = None
        self.shadow = None
        self._lock = threading.RLock()
        self._store = None

    def __getattribute__(self, name):
        if not name.startswith("_") and name not in Int8Corpus._SERVED and callable(getattr(DeviceCorpus, name, None)):
            raise NotImplementedError(f"{name}: a stand-alone int8 corpus serves search_approx(rescore=False) only")
        return object.__getattribute__(self, name)

    @property
    def n_rows(self) -> int:
        return int(self.i8_codes.shape[0])

    @property
    def dim(self) -> int:
        return int(self.i8_codes.shape[1])

    @property
    def is_bf16(self) -> bool:
        return False

    def corpus_bytes(self) -> int:
        return self.i8_codes.numel() + 4 * self.i8_scales.numel()

    def search_approx_device(self, q_dev, k: int, eta: float, entropy_pref: float, candidates: Optional[int] = None,
                             rescore: bool = False, out_ids=None, out_scores=None):
        if rescore:
            raise NotImplementedError("a stand-alone int8 corpus has no fp32 rows to re-score from: pass rescore=False")
        return DeviceCorpus.search_approx_device(self, q_dev, k, eta, entropy_pref, candidates, False, out_ids, out_scores)

    def search_approx(self, queries: ArrayLike, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                      candidates: Optional[int] = None, rescore: bool = False,
                      batch_pass: Optional[bool] = None) -> Tuple[np.ndarray, np.ndarray]:
        if rescore:
            raise NotImplementedError("a stand-alone int8 corpus has no fp32 rows to re-score from: pass rescore=False")
        return DeviceCorpus.search_approx(self, queries, k, eta, entropy_pref, candidates, False, batch_pass=batch_pass)


class PipelinedSearcher:
    """Two query batches in flight on one GPU (throughput mode).

    Batch i's scan runs on ``scan_stream``; its finish (select, blend, top-k — or, for a doc-id
    shard, the candidate records) runs on ``finish_stream`` from one of two workspaces, so it
    overlaps the scan of batch i+1.  Scans themselves stay back to back on one stream: nothing
    competes with the corpus stream for HBM.  ``submit`` only enqueues; call ``drain`` before
    reading the outputs.

    ``dewi_knn_scan`` / ``dewi_knn_finish`` take the same kernels as the one-call search (a batch of
    queries: the matrix-core passes); a query such a pass refuses is repaired by ``dewi_knn_finish`` itself
    (ABI 5), from the query tensor that was SUBMITTED — which must therefore stay untouched until the finish
    step has run (``drain``, or an event on ``finish_stream``): a caller that reuses one staging buffer for
    its queries submits a clone.  The workspace size and the path are fixed from the
    submitting thread's tuning (``_engine.tuning`` is thread-local): construct and submit from one thread.
    """

    def __init__(self, corpus: DeviceCorpus, k: int, eta: float, entropy_pref: float, n_queries: int = 1,
                 n_candidates: Optional[int] = None, finish_stream=None, depth: int = 2, scan_streams: int = 1):
        torch = _torch()
        self.corpus = corpus
        self.k, self.eta, self.pref, self.b = int(k), float(eta), float(entropy_pref), int(n_queries)
        self.c = int(n_candidates) if n_candidates is not None else min(2 * self.k, corpus.n_rows)
        self._lib = corpus._lib
        need = self._need = library_size(self._lib.dewi_knn_workspace_bytes, corpus.n_rows, corpus.dim, self.b,
                                         cut_size(self.k, self.c, corpus.n_rows))
        with torch.cuda.device(corpus.device):
            # scan_streams > 1: consecutive scans alternate between streams, so the tail of one (block merge,
            # last workgroups) overlaps the ramp of the next (query preparation) — small shards only
            # (alternating priorities: streams of different priority never share a hardware queue, so the
            # overlap does not depend on how the runtime happens to map streams to queues)
            self._scan_streams = [torch.cuda.Stream(priority=-(j % 2)) for j in range(max(1, int(scan_streams)))]
            self.scan_stream = self._scan_streams[0]
            self.finish_stream = finish_stream if finish_stream is not None else torch.cuda.Stream()
            self.depth = max(2, int(depth))   # workspaces in rotation = scans that may run ahead of their finish
            self._ws = [torch.empty(need, dtype=torch.uint8, device=corpus.device) for _ in range(self.depth)]
            self._scan_done = [torch.cuda.Event() for _ in range(self.depth)]
            self._finish_done = [torch.cuda.Event() for _ in range(self.depth)]
        self._i = 0
        self._elem = corpus._elem
        self._space = nat.SPACE_CODES[corpus.space]
        self._emb, self._dewi, self._ent = nat.ptr(corpus.emb), nat.ptr(corpus.dewi32), nat.ptr(corpus.ent32)
        self._s_scans = [int(st.cuda_stream) for st in self._scan_streams]
        self._s_fin = int(self.finish_stream.cuda_stream)

    def submit(self, q_dev, out_ids=None, out_scores=None, out_records=None) -> None:
        """Enqueue one query batch.  Final results go to (out_ids, out_scores); with ``out_records``
        (int32 [B, c, 4]) the shard's candidate records are written instead."""
        i = self._i
        slot = i % self.depth
        self._i = i + 1
        c = self.corpus
        which = i % len(self._scan_streams)
        scan_stream = self._scan_streams[which]
        if i >= self.depth:
            scan_stream.wait_event(self._finish_done[slot])            # workspace `slot` is free again
        rc = self._lib.dewi_knn_scan(self._emb, self._elem, c.n_rows, c.dim, q_dev.data_ptr(), self.b, self.c,
                                     self._space, self._ws[slot].data_ptr(), self._need, self._s_scans[which])
        if rc:
            nat.check(rc)
        self._scan_done[slot].record(scan_stream)
        self.finish_stream.wait_event(self._scan_done[slot])
        if out_records is None:
            rc = self._lib.dewi_knn_finish(self._ws[slot].data_ptr(), self._need, self._emb, self._elem, c.n_rows, c.dim,
                                           q_dev.data_ptr(), self.b, self.c, self._space, self.k, self.eta, self.pref, self._dewi,
                                           self._ent, c.id_offset, out_ids.data_ptr(), out_scores.data_ptr(), 0, self._s_fin)
        else:
            rc = self._lib.dewi_knn_finish(self._ws[slot].data_ptr(), self._need, self._emb, self._elem, c.n_rows, c.dim,
                                           q_dev.data_ptr(), self.b, self.c, self._space, 0, 0.0, 0.0, self._dewi, self._ent,
                                           c.id_offset, 0, 0, out_records.data_ptr(), self._s_fin)
        if rc:
            nat.check(rc)
        self._finish_done[slot].record(self.finish_stream)

    def drain(self) -> None:
        for st in self._scan_streams:
            st.synchronize()
        self.finish_stream.synchronize()


# scratch of the large merge, one buffer per (device, stream): reuse is ordered by the stream it is used on, so two streams
# (the current stream beside a PipelinedSearcher / sharded finish stream) or two threads never share one
_merge_ws: Dict[object, "torch.Tensor"] = {}


def merge_rerank_device(lists, n_candidates: int, k: int, eta: float, entropy_pref: float, out_ids=None,
                        out_scores=None):
    """lists: int32 [n_lists, B, list_len, 4] candidate records (the all-gather result)."""
    torch = _torch()
    lib = nat.load_library()
    n_lists, b, list_len = int(lists.shape[0]), int(lists.shape[1]), int(lists.shape[2])
    if out_ids is None:
        out_ids = torch.empty((b, k), dtype=torch.int64, device=lists.device)
    if out_scores is None:
        out_scores = torch.empty((b, k), dtype=torch.float32, device=lists.device)
    # up to 2048 records per query are merged in LDS; beyond that (k > 128 at eight shards) through a scratch buffer
    need = int(lib.dewi_merge_workspace_bytes(n_lists, b, list_len, int(n_candidates)))
    ws = None
    if need:
        key = (lists.device, int(torch.cuda.current_stream(lists.device).cuda_stream))
        ws = _merge_ws.get(key)
        if ws is None or ws.numel() < need:
            if len(_merge_ws) > 16:
                _merge_ws.clear()
            # (a buffer that is outgrown is only dropped here: the caching allocator keeps its memory stream-ordered, so a
            # merge still running on this stream finishes on it before anything else of this stream can take the block)
            ws = _merge_ws[key] = torch.empty(need, dtype=torch.uint8, device=lists.device)
    rc = lib.dewi_merge_rerank(nat.ptr(lists), n_lists, b, list_len, int(n_candidates), int(k), float(eta),
                               float(entropy_pref), nat.ptr(out_ids), nat.ptr(out_scores),
                               nat.ptr(ws) if ws is not None else None, need, nat.stream_ptr())
    nat.check(rc)
    return out_ids, out_scores


def records_to_numpy(recs) -> np.ndarray:
    """int32 [.., 4] record tensor -> structured host array (sim, dewi, ent, id)."""
    a = recs.detach().cpu().numpy()
    dt = np.dtype([("sim", np.float32), ("dewi", np.float32), ("ent", np.float32), ("id", np.int32)])
    return np.ascontiguousarray(a).view(dt).reshape(a.shape[:-1])


def timing(every) -> None:
    """Bracket every ``every``-th scan with hipEvents (True == 1: every scan; False / 0: off)."""
    nat.check(nat.load_library().dewi_timing_enable(int(every)))


def timing_read() -> Tuple[float, int]:
    ms = ctypes.c_double(0.0)
    n = ctypes.c_int(0)
    nat.check(nat.load_library().dewi_timing_read(ctypes.byref(ms), ctypes.byref(n)))
    return float(ms.value), int(n.value)


def prepare_queries_bf16(q_dev, space: str = "cosine"):
    """The query-preparation kernel of the batched matrix-core path on its own: normalised (cosine) bf16
    queries [B, d] on the device (``dewi_prepare_queries_bf16``).  For parity tests and diagnostics."""
    torch = _torch()
    lib = nat.load_library()
    q = q_dev.to(dtype=torch.float32).contiguous()
    out = torch.empty(q.shape, dtype=torch.bfloat16, device=q.device)
    with torch.cuda.device(q.device):
        nat.check(lib.dewi_prepare_queries_bf16(nat.ptr(q), int(q.shape[0]), int(q.shape[1]), nat.SPACE_CODES[space],
                                                nat.ptr(out), nat.stream_ptr()))
    return out


def tuning(scan_blocks: int = 0, rows_per_iter: int = 0, nontemporal: int = -1, batched_mfma: int = 1) -> None:
    """Launch-shape overrides of the CALLING THREAD (the library keeps them thread-local).
    batched_mfma: 0 row kernels only; 1 (default) cosine batches on the matrix cores, ``space="l2"`` batches over an fp32
    corpus too (exact-refine mode: error-widened cut, candidates re-scored with the row kernels' arithmetic); 2 also l2
    batches over a bf16 corpus, unrefined (2<e,q> - ||e||^2 - ||q||^2: absolute error ~ulp(||e||^2+||q||^2) —
    near-duplicates of a query lose their near-zero distance; not the parity path)."""
    _thread_tuning.epoch = next(_tuning_epochs)      # this thread's cached workspace sizes are asked for again
    nat.check(nat.load_library().dewi_tuning_set(int(scan_blocks), int(rows_per_iter), int(nontemporal),
                                                 int(batched_mfma)))

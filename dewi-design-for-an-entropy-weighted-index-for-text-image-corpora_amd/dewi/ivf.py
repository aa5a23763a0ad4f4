"""``IVFIndex``: approximate search that scans only the rows of the k-means cells nearest to the query (IVF-Flat).

The corpus stays exactly what ``ExactIndex`` keeps (same row order, ids, payload columns, files).  On top of it ``build``
trains ``nlist`` centroids (Lloyd's k-means on the device, in torch: plumbing, once per build), assigns every row to its
nearest centroid and sorts the rows into per-cell lists (``dewi_ivf_lists_build``).  A search is three steps on one stream:

1. coarse: the ``nprobe`` nearest centroids of every query — the exact search over the centroid matrix, ids left on the device;
2. ``dewi_ivf_probe_prepare``: the rows of those cells as a prepared filter, one per group of 8 queries (so that a pass
   streams the union of 8 queries' cells, not of the whole batch), with one word of query bits per row;
3. the filtered search entry points on that buffer (``dewi_knn_rerank_filtered`` for one query,
   ``dewi_knn_rerank_query_filtered`` for a group).

So query j's answer is, bit for bit, ``ExactIndex.search(q_j, k, ..., filter=<rows of its probed cells>)``: the reference's
search on those rows only.  ``nprobe >= nlist`` probes every row and returns the exact result.

``search_probe_filtered*`` run the same three steps under a user filter: step 2 is ``dewi_ivf_probe_prepare_filtered``, which
drops the probed rows the filter does not allow on the device, and query j's answer is the search on what is left.
"""
from __future__ import annotations

import ctypes
import json
import math
from pathlib import Path
from typing import Any, Optional, Tuple, Union

import numpy as np

from .backends import ExactIndex, SearchResult

IVF_FORMAT_VERSION = 1
MAX_CELLS = 65536          # dewi_hip.h: 1 <= n_cells <= min(65536, n_rows)
PROBE_GROUP = 8            # queries that share one pass over the union of their cells (what the QMASK passes take)


def default_nlist(n_rows: int) -> int:
    return min(4096, max(1, int(round(math.sqrt(n_rows)))))


def default_nprobe(nlist: int) -> int:
    return max(1, nlist // 64)


class _IvfState:
    """What a built IVF index keeps on the device: centroids (as a small exact corpus), the cell of every row, the lists."""

    __slots__ = ("nlist", "buckets", "centroids", "coarse", "assign", "lists", "corpus_id")


class IVFIndex(ExactIndex):
    """IVF-Flat over an ``ExactIndex`` corpus (fp32 rows; ``int8_codes=True`` keeps an int8 copy for approximate probes).

    ``int8_codes=True`` (cosine, ``dim % 16 == 0`` up to 4096: checked here): ``build`` keeps the int8 copy of the rows
    (``DeviceCorpus.enable_int8_shadow``, +25 % memory) and ``search`` / ``search_batch`` / ``search_device`` take
    ``approx``: step 3 then picks each query's cut by the int8 scores of its probed rows — a quarter of the bytes —,
    re-scores it from the fp32 rows (``rescore=False``: not) and blends as ever, so query j's answer is
    ``ExactIndex.search_approx_filtered`` on the rows of its cells.  ``approx=None`` takes that route iff the index has
    codes, ``similarity == "ip"``, there is no ``filter``, the cut is at most 1024 and the batch at most
    ``APPROX_AUTO_MAX_BATCH``; ``approx=False`` is the fp32 probe, bit for bit.  The int8 probe is SLOWER than the fp32 probe
    wherever the probe is short (fixed cost: profiles/r14/int8_lists/).  ``remove`` / ``upsert*`` mark the copy stale (the
    next approximate search re-quantises); ``load(path, int8_codes=True)`` re-quantises, nothing changes on disk.
    ``int8_shadow=True`` (``ExactIndex``'s unfiltered int8 route) and ``binary_shadow=True`` (its 1-bit route) are refused.

    ``nlist=None``: ``min(4096, max(1, round(sqrt(N))))`` at build; ``nprobe=None``: ``max(1, nlist // 64)``.  Training:
    ``train_iters`` rounds of k-means from ``nlist`` distinct rows drawn with ``np.random.RandomState(train_seed)``, at most
    ``max_train_rows`` (default ``256 * nlist``) sampled rows per round, every row in the final assignment; spherical
    (centroids re-normalised every round) for ``space="cosine"``, plain means for ``"l2"``; an empty cell keeps its previous
    centroid.  The same corpus and seed give the same cells on the same machine.  ``add`` + ``build`` after a build retrains.

    ``range_search`` / ``range_search_batch`` are ``ExactIndex``'s, unchanged: they scan EVERY row (or every row of
    ``filter``) and are exact — the cells are not consulted and there is no ``nprobe`` argument.  A range search over the
    probed cells only is not part of this build.

    ``duplicate_groups`` / ``dedup_filter`` are inherited as well and exact.  ``search(..., filter=dedup_filter(...))`` on
    this class is what any user filter is there: the parent's exact filtered search over the whole allow-list, not a probe.

    A user filter TOGETHER with the probe is ``search_probe_filtered`` / ``search_probe_filtered_batch`` /
    ``search_probe_filtered_device``: ``filter=`` is whatever ``search(filter=)`` takes (a mask, doc ids, rows, a prepared
    ``DeviceFilter``, ``dedup_filter(...)``, per-query masks or ``DeviceQueryFilters``), and step 2 becomes
    ``dewi_ivf_probe_prepare_filtered``: the probed cells are expanded and the rows the user does not allow are dropped on
    the device, at a cost proportional to the probed rows.  Query j's answer is the exact search on (rows of its cells) ∩
    (its allow-list); ``widen=True`` doubles ``nprobe`` for the queries that a selective filter leaves below the cut;
    ``approx=True`` scans the int8 codes (``int8_codes=True``).  ``search`` / ``search_batch`` do not route there by
    themselves (measurements: profiles/r15/ivf_filtered/).

    ``search_diverse`` / ``search_diverse_batch`` are ``ExactIndex``'s too, in their EXACT form: the candidate pool is the
    exact cut over every row, not over the probed cells, and there is no ``nprobe`` argument.  A diverse search over an IVF
    probe is not part of this build.  ``search_collapsed`` / ``search_collapsed_batch`` are inherited in the same EXACT form
    (the pool is the exact cut over every row, or over every row of ``filter``; no ``nprobe``): a collapsed search over a
    probe is not part of this build.  ``search_by_examples`` is inherited in its EXACT form as well (every row, or every row of
    ``filter``, is scored against the examples; no ``nprobe``).

    ``remove`` / ``upsert`` / ``upsert_batch`` / ``upsert_batch_columns`` maintain the cells instead of retraining: the
    centroids stay as trained, a surviving document keeps its cell, a replaced or appended one goes to the centroid nearest to
    its stored row, and the lists are rebuilt.  The cells therefore DRIFT from what k-means would give the changed corpus as
    documents come and go; ``build()`` retrains, as ever.  A removal that would leave fewer documents than cells is refused.
    """

    def __init__(self, dim: int, space: str = "cosine", nlist: Optional[int] = None, nprobe: Optional[int] = None,
                 train_iters: int = 10, train_seed: int = 0, max_train_rows: Optional[int] = None, **kwargs: Any):
        if nlist is not None and not (1 <= int(nlist) <= MAX_CELLS):
            raise ValueError(f"nlist must lie in [1, {MAX_CELLS}], got {nlist}")
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"nprobe must be at least 1, got {nprobe}")
        if int(train_iters) < 0:
            raise ValueError(f"train_iters must not be negative, got {train_iters}")
        if max_train_rows is not None and int(max_train_rows) < 1:
            raise ValueError(f"max_train_rows must be at least 1, got {max_train_rows}")
        if kwargs.get("int8_shadow"):
            raise ValueError("IVFIndex does not take int8_shadow (the unfiltered int8 route scans every row): "
                             "int8_codes=True keeps the int8 copy for the probes")
        if kwargs.get("binary_shadow"):
            raise ValueError("IVFIndex does not take binary_shadow (the binary route scans every row)")
        int8_codes = bool(kwargs.pop("int8_codes", False))
        if int8_codes:
            from ._engine import check_int8_shape
            check_int8_shape(space, False, dim)
        super().__init__(dim, space, **kwargs)
        self._int8_codes = int8_codes
        self.nlist = None if nlist is None else int(nlist)
        self.nprobe = None if nprobe is None else int(nprobe)
        self.train_iters = int(train_iters)
        self.train_seed = int(train_seed)
        self.max_train_rows = None if max_train_rows is None else int(max_train_rows)
        self._ivf: Optional[_IvfState] = None
        self._ivf_loaded = None                   # (centroids, assign) read by load(): taken instead of training
        self._probe_buf = None                    # one probe buffer and one search workspace, both only ever grow
        self._ivf_ws = None

    # ---------------------------------------------------------------- build
    def build(self, **kwargs: Any) -> None:
        """``ExactIndex.build`` (the corpus in its row order), then the centroids, the assignment and the cell lists."""
        super().build(**kwargs)
        self._build_ivf()

    def _ensure_built(self) -> None:
        super()._ensure_built()
        if self._ivf is None or self._ivf.corpus_id != self._corpus.corpus_id:
            self._build_ivf()

    def _build_ivf(self) -> None:
        import torch
        from . import _native as nat
        from ._engine import DeviceCorpus
        corpus = self._corpus
        if corpus.is_bf16:
            raise NotImplementedError("IVFIndex serves fp32 corpora (bf16: not in this build)")
        lib = nat.load_library()
        n, dev = corpus.n_rows, corpus.device
        loaded, self._ivf_loaded = self._ivf_loaded, None
        with torch.cuda.device(dev):
            if loaded is not None and loaded[1].shape[0] == n and loaded[0].shape[1] == self.dim:
                centroids = torch.from_numpy(np.ascontiguousarray(loaded[0], dtype=np.float32)).to(dev)
                assign = torch.from_numpy(np.ascontiguousarray(loaded[1], dtype=np.int32)).to(dev)
                nlist = int(centroids.shape[0])
            else:
                nlist = default_nlist(n) if self.nlist is None else self.nlist
                if nlist > n:
                    raise ValueError(f"nlist = {nlist} exceeds the {n} rows of the corpus")
                centroids, assign = self._train(corpus.emb, nlist)
            st = _IvfState()
            st.nlist = nlist
            st.buckets = int(lib.dewi_ivf_buckets(self.dim, 0))
            self._make_lists(st, assign, n)
            zeros = torch.zeros(nlist, dtype=torch.float32, device=dev)
            st.centroids, st.assign = centroids, assign
            st.coarse = DeviceCorpus(centroids, zeros, zeros.clone(), self.space)
            st.corpus_id = corpus.corpus_id
            if self._int8_codes:
                corpus.enable_int8_shadow()       # the int8 copy the approximate probes scan (remove / upsert* mark it stale)
        self._ivf = st

    def _make_lists(self, st: _IvfState, assign, n: int) -> None:
        """``st.lists``: the per-cell row lists of ``assign`` (int32 [n] on the device), by ``dewi_ivf_lists_build``."""
        import torch
        from . import _native as nat
        lib = nat.load_library()
        nlist = st.nlist
        need = int(lib.dewi_ivf_lists_bytes(n, self.dim, 0, nlist))
        if need == 0 or st.buckets == 0:
            raise nat.NativeLibraryError(f"dewi_ivf_lists_bytes returned 0 for {n} x {self.dim}, {nlist} cells")
        st.lists = torch.empty(need, dtype=torch.uint8, device=assign.device)
        nat.check(lib.dewi_ivf_lists_build(0, n, self.dim, nlist, nat.ptr(assign), nat.ptr(st.lists), need, nat.stream_ptr()))
        words = st.lists.view(torch.int32)
        dropped = int(words[nlist * st.buckets + 1 + n].item())           # the error word (synchronises)
        if dropped:
            raise ValueError(f"{dropped} rows are assigned to cells outside [0, {nlist})")

    # ---------------------------------------------------------------- remove / upsert in place
    # Mutations maintain the cells instead of retraining: the centroids are untouched, a surviving row keeps its cell (the
    # cell column travels with the row mover), a replaced or appended row goes to the centroid nearest to its stored row, and
    # the lists are rebuilt from the cell column.  The cells therefore DRIFT from what k-means would give the changed corpus
    # as documents come and go; ``build()`` retrains, as ever.
    def _check_removal(self, n_keep: int) -> None:
        super()._check_removal(n_keep)
        if self._ivf is not None and n_keep < self._ivf.nlist:
            raise ValueError(f"cannot remove down to {n_keep} documents: the index has {self._ivf.nlist} cells")

    def _corpus_remove(self, rows: np.ndarray):
        import torch
        st, corpus = self._ivf, self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            src, dst = corpus.remove_rows(rows, aux=st.assign)
            st.assign = st.assign[: corpus.n_rows].contiguous()
            self._make_lists(st, st.assign, corpus.n_rows)
            st.corpus_id = corpus.corpus_id
        return src, dst

    def _corpus_put(self, rows: np.ndarray, embeddings, triple) -> None:
        import torch
        st, corpus = self._ivf, self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            super()._corpus_put(rows, embeddings, triple)
            at = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(corpus.device)
            cells = self._assign(corpus.emb.index_select(0, at), st.centroids).to(torch.int32)
            grown = corpus.n_rows - int(st.assign.shape[0])
            if grown > 0:
                st.assign = torch.cat([st.assign, torch.zeros(grown, dtype=torch.int32, device=corpus.device)])
            st.assign[at] = cells
            self._make_lists(st, st.assign, corpus.n_rows)
            st.corpus_id = corpus.corpus_id

    def _assign(self, X, C):
        """Nearest centroid of every row of X (int64): largest inner product (cosine) / smallest distance (l2)."""
        import torch
        out = torch.empty(X.shape[0], dtype=torch.int64, device=X.device)
        bias = None if self.space != "l2" else (C * C).sum(dim=1)
        ct = C.t().contiguous()
        step = max(1024, (1 << 26) // max(int(C.shape[0]), 1))               # <= 256 MiB of scores at a time
        for s in range(0, int(X.shape[0]), step):
            sc = torch.mm(X[s:s + step], ct)
            if bias is not None:
                sc = 2.0 * sc - bias
            out[s:s + step] = torch.argmax(torch.nan_to_num(sc, nan=-float("inf")), dim=1)
        return out

    def _train(self, X, nlist: int):
        import torch
        n = int(X.shape[0])
        rs = np.random.RandomState(self.train_seed)
        init = np.sort(rs.choice(n, nlist, replace=False))
        C = torch.nan_to_num(X[torch.from_numpy(init).to(X.device)].clone())
        cap = 256 * nlist if self.max_train_rows is None else self.max_train_rows
        for _ in range(self.train_iters):
            if n > cap:
                pick = torch.from_numpy(np.sort(rs.choice(n, cap, replace=False))).to(X.device)
                Xs = X[pick]
            else:
                Xs = X
            a = self._assign(Xs, C)
            # sorted form of the update (no floating-point atomics: the same cells on every run)
            order = torch.argsort(a, stable=True)
            counts = torch.bincount(a, minlength=nlist)
            sums = torch.segment_reduce(torch.nan_to_num(Xs[order]), "sum", lengths=counts, axis=0)
            means = sums / counts.clamp(min=1).to(sums.dtype).unsqueeze(1)
            keep = counts > 0
            if self.space == "cosine":
                norm = torch.linalg.vector_norm(means, dim=1, keepdim=True)
                keep = keep & (norm.squeeze(1) > 0)
                means = means / norm.clamp(min=1e-30)
            C = torch.where(keep.unsqueeze(1), means, C)                        # an empty cell keeps its previous centroid
        return C.contiguous(), self._assign(X, C).to(torch.int32).contiguous()

    def _invalidate(self) -> None:
        super()._invalidate()
        self._ivf_loaded = None

    # ---------------------------------------------------------------- introspection
    @property
    def centroids(self) -> np.ndarray:
        self._ensure_built()
        return self._ivf.centroids.cpu().numpy()

    @property
    def cell_of_row(self) -> np.ndarray:
        self._ensure_built()
        return self._ivf.assign.cpu().numpy()

    @property
    def cell_sizes(self) -> np.ndarray:
        return np.bincount(self.cell_of_row, minlength=self._ivf.nlist).astype(np.int64)

    def cell_lists(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """(offsets uint32 [nlist * G + 1], rows uint32 [N], G): the device's cell lists as ``dewi_ivf_lists_build`` wrote
        them — segment (cell, b) holds the cell's rows with row mod G == b, ascending."""
        self._ensure_built()
        import torch
        st = self._ivf
        words = st.lists.view(torch.int32).cpu().numpy().view(np.uint32)
        bins = st.nlist * st.buckets
        return words[: bins + 1].copy(), words[bins + 1: bins + 1 + self._corpus.n_rows].copy(), st.buckets

    def _resolve_nprobe(self, nprobe: Optional[int], nlist: int) -> int:
        if nprobe is None:
            nprobe = self.nprobe
        if nprobe is None:
            nprobe = default_nprobe(nlist)
        if int(nprobe) < 1:
            raise ValueError(f"nprobe must be at least 1, got {nprobe}")
        return min(int(nprobe), nlist)

    def probe(self, queries: np.ndarray, nprobe: Optional[int] = None) -> np.ndarray:
        """The cells each query probes: int64 [B, nprobe], nearest first (the coarse step on its own)."""
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"nprobe must be at least 1, got {nprobe}")
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        npb = self._resolve_nprobe(nprobe, self._ivf.nlist)
        ids, _ = self._ivf.coarse.search(q, npb, 0.0, 0.0, candidates=npb)
        return ids

    # ---------------------------------------------------------------- search
    def _prepare_probe(self, probe_ids, b: int, nprobe: int):
        """``dewi_ivf_probe_prepare`` into the index's probe buffer -> (|U| per group, |F_j| per query, bytes per group)."""
        import torch
        from . import _native as nat
        lib, st, corpus = nat.load_library(), self._ivf, self._corpus
        need = int(lib.dewi_ivf_probe_bytes(corpus.n_rows, self.dim, 0, b, PROBE_GROUP))
        stride = int(lib.dewi_ivf_probe_group_bytes(corpus.n_rows, self.dim, 0, PROBE_GROUP))
        if need == 0 or stride == 0:
            raise nat.NativeLibraryError(f"dewi_ivf_probe_bytes returned 0 for {b} queries")
        if self._probe_buf is None or self._probe_buf.numel() < need or self._probe_buf.device != corpus.device:
            self._probe_buf = torch.empty(need, dtype=torch.uint8, device=corpus.device)
        n_groups = (b + PROBE_GROUP - 1) // PROBE_GROUP
        n_union = (ctypes.c_int64 * n_groups)()
        n_allowed = (ctypes.c_int64 * b)()
        nat.check(lib.dewi_ivf_probe_prepare(0, corpus.n_rows, self.dim, nat.ptr(st.lists), st.nlist, nat.ptr(probe_ids), b,
                                             nprobe, PROBE_GROUP, nat.ptr(self._probe_buf), self._probe_buf.numel(), n_union,
                                             n_allowed, nat.stream_ptr()))
        return list(n_union), list(n_allowed), stride

    def _workspace_for(self, n_union: int, nq: int, c: int):
        # one grow-only buffer, sized on every call: (n_union, nq) change with every probe, so there is nothing to cache by
        import torch
        from ._engine import library_size
        need = library_size(self._corpus._lib.dewi_knn_filtered_workspace_bytes, n_union, self.dim, nq, c)
        if self._ivf_ws is None or self._ivf_ws.numel() < need or self._ivf_ws.device != self._corpus.device:
            self._ivf_ws = torch.empty(need, dtype=torch.uint8, device=self._corpus.device)
        return self._ivf_ws

    def _search_groups(self, q_dev, n_union, n_allowed, stride: int, k: int, c: int, candidates: Optional[int], sim: int,
                       eta: float, pref: float, out_ids, out_scores) -> None:
        """Step 3 on a prepared probe buffer whose every query holds at least c rows (one query: at least k)."""
        from . import _native as nat
        corpus, lib = self._corpus, self._corpus._lib
        b = int(q_dev.shape[0])
        space = nat.SPACE_CODES[self.space]
        n_cand = 0 if candidates is None else int(candidates)
        for g, q0 in enumerate(range(0, b, PROBE_GROUP)):
            nq = min(PROBE_GROUP, b - q0)
            buf = self._probe_buf[g * stride:]
            ws = self._workspace_for(n_union[g], nq, c)
            if nq == 1:
                rc = lib.dewi_knn_rerank_filtered(
                    nat.ptr(corpus.emb), 0, corpus.n_rows, self.dim, nat.ptr(buf), n_union[g], nat.ptr(q_dev[q0:q0 + 1]), 1,
                    nat.ptr(corpus.dewi32), nat.ptr(corpus.ent32), k, n_cand, sim, eta, pref, space,
                    nat.ptr(out_ids[q0:q0 + 1]), nat.ptr(out_scores[q0:q0 + 1]), nat.ptr(ws), ws.numel(), nat.stream_ptr())
            else:
                counts = (ctypes.c_int64 * nq)(*n_allowed[q0:q0 + nq])
                rc = lib.dewi_knn_rerank_query_filtered(
                    nat.ptr(corpus.emb), 0, corpus.n_rows, self.dim, nat.ptr(buf), n_union[g], counts, nat.ptr(q_dev[q0:q0 + nq]),
                    nq, nat.ptr(corpus.dewi32), nat.ptr(corpus.ent32), k, n_cand, sim, eta, pref, space,
                    nat.ptr(out_ids[q0:q0 + nq]), nat.ptr(out_scores[q0:q0 + nq]), nat.ptr(ws), ws.numel(), nat.stream_ptr())
            nat.check(rc)

    #: largest batch ``approx=None`` sends through the int8 probe (``None``: every batch).  Measured at 1 M x 768, nlist 1024,
    #: k = 10 (profiles/r14/int8_lists/): 32 queries lose at nprobe 1 / 4 / 16 (0.51 / 0.53 / 0.80 ms against 0.29 / 0.39 /
    #: 0.71 ms on the fp32 rows) and gain 3 % at nprobe 64; batches of 2 .. 31 have not been measured.  One query gains only
    #: where the probe is long (nprobe 64, 109 k rows: 0.146 against 0.162 ms) and loses 0.024 ms of fixed cost below.
    APPROX_AUTO_MAX_BATCH = 1

    def _use_approx_probe(self, approx: Optional[bool], similarity: str, filter, k: int, candidates: Optional[int],
                          n_queries: int = 1) -> bool:
        """Whether a search scans the int8 codes of the probed cells.  ``True``: it must (``ValueError`` without codes, with a
        ``filter`` or with a similarity transform); ``None``: where the index has codes and the route serves the call (no
        filter, no transform, a cut of at most 1024, at most ``APPROX_AUTO_MAX_BATCH`` queries); ``False``: never."""
        from . import _native as nat
        if approx is None:
            cap = self.APPROX_AUTO_MAX_BATCH
            if not self._int8_codes or filter is not None or similarity != "ip" or (cap is not None and int(n_queries) > cap):
                return False
            return (2 * int(k) if candidates is None else int(candidates)) <= nat.I8_MAX_CANDIDATES
        if not approx:
            return False
        if not self._int8_codes:
            raise ValueError("approx=True needs an IVFIndex built with int8_codes=True (int8_shadow=True is ExactIndex's "
                             "unfiltered route, which an IVFIndex does not have)")
        if filter is not None:
            raise ValueError("approx=True does not take a filter: a user filter together with an IVF probe is not supported")
        if similarity != "ip":
            raise ValueError("approx=True does not take a similarity transform")
        return True

    def _search_groups_i8(self, q_dev, n_union, n_allowed, stride: int, k: int, c: int, rescore: bool, eta: float, pref: float,
                          out_ids, out_scores) -> None:
        """Step 3 on the int8 codes: per group the records of the c best rows by int8 score
        (``dewi_knn_candidates_i8_query_filtered``; a group of one: ``dewi_knn_candidates_i8_filtered``), re-scored from the
        fp32 rows unless ``rescore`` is off, then ``dewi_merge_rerank``.  Every query holds at least c rows."""
        import torch
        from . import _native as nat
        from ._engine import library_size
        corpus, lib = self._corpus, self._corpus._lib
        codes, scales = corpus._int8()
        b = int(q_dev.shape[0])
        for g, q0 in enumerate(range(0, b, PROBE_GROUP)):
            nq = min(PROBE_GROUP, b - q0)
            buf = self._probe_buf[g * stride:]
            need = library_size(lib.dewi_knn_i8_filtered_workspace_bytes, n_union[g], self.dim, nq, c)
            if self._ivf_ws is None or self._ivf_ws.numel() < need or self._ivf_ws.device != corpus.device:
                self._ivf_ws = torch.empty(need, dtype=torch.uint8, device=corpus.device)
            ws = self._ivf_ws
            recs = torch.empty((nq, c, 4), dtype=torch.int32, device=corpus.device)
            q_g = q_dev[q0:q0 + nq]
            if nq == 1:
                rc = lib.dewi_knn_candidates_i8_filtered(
                    nat.ptr(codes), nat.ptr(scales), corpus.n_rows, self.dim, nat.ptr(buf), n_union[g], nat.ptr(q_g), 1,
                    nat.ptr(corpus.dewi32), nat.ptr(corpus.ent32), c, 0, nat.ptr(recs), nat.ptr(ws), ws.numel(), nat.stream_ptr())
            else:
                counts = (ctypes.c_int64 * nq)(*n_allowed[q0:q0 + nq])
                rc = lib.dewi_knn_candidates_i8_query_filtered(
                    nat.ptr(codes), nat.ptr(scales), corpus.n_rows, self.dim, nat.ptr(buf), n_union[g], counts, nat.ptr(q_g), nq,
                    nat.ptr(corpus.dewi32), nat.ptr(corpus.ent32), c, 0, nat.ptr(recs), nat.ptr(ws), ws.numel(), nat.stream_ptr())
            nat.check(rc)
            corpus._rerank_records(q_g, recs, rescore, k, eta, pref, out_ids[q0:q0 + nq], out_scores[q0:q0 + nq])

    def search_device(self, q_dev, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0, candidates: Optional[int] = None,
                      similarity: str = "ip", nprobe: Optional[int] = None, approx: Optional[bool] = None, rescore: bool = True):
        """The three steps for fp32 queries [B, dim] on the corpus's device -> (ids int64 [B, k], scores fp32 [B, k]) device
        tensors.  Synchronises the current stream once (the probe's row counts come back to the host to plan the scan); the
        search itself is left enqueued.  A query whose cells hold fewer than k rows fills the rest of its row with id -1 /
        score NaN.  One caller at a time (shared buffers).  ``approx`` / ``rescore``: see ``search_batch``."""
        import torch
        from . import _native as nat
        from ._engine import approx_cut, check_search_args, cut_size, default_outputs, empty_result
        use_i8 = self._use_approx_probe(approx, similarity, None, k, candidates, int(q_dev.shape[0]))
        self._ensure_built()
        corpus, st = self._corpus, self._ivf
        if corpus.is_bf16:
            raise NotImplementedError("IVFIndex serves fp32 corpora (bf16: not in this build)")
        npb = self._resolve_nprobe(nprobe, st.nlist)
        b, k = check_search_args(q_dev.shape, self.dim, k, candidates, similarity)
        if k <= 0:
            return empty_result(b, corpus.device)
        if candidates is not None and int(candidates) < k:
            raise ValueError(f"candidates = {candidates} must be at least k = {k}")
        c = cut_size(k, candidates)
        if use_i8 and c > nat.I8_MAX_CANDIDATES:
            approx_cut(k, candidates, c)             # raises: the int8 route re-ranks at most 1024 candidates
        sim, eta, pref = nat.SIM_CODES[similarity], float(eta), float(entropy_pref)
        out_ids, out_scores = default_outputs(b, k, corpus.device)
        probe_ids, _ = st.coarse.search_device(q_dev, npb, 0.0, 0.0, candidates=npb)
        n_union, n_allowed, stride = self._prepare_probe(probe_ids, b, npb)

        def groups(q, n_union, n_allowed, stride, kk, cc, o_ids, o_sc):
            if use_i8:
                self._search_groups_i8(q, n_union, n_allowed, stride, kk, cc, rescore, eta, pref, o_ids, o_sc)
            else:
                self._search_groups(q, n_union, n_allowed, stride, kk, cc, candidates, sim, eta, pref, o_ids, o_sc)

        short = [j for j in range(b) if n_allowed[j] < c]
        if not short:
            groups(q_dev, n_union, n_allowed, stride, k, c, out_ids, out_scores)
            return out_ids, out_scores
        # queries whose cells hold fewer rows than the cut leave the shared passes: one list each, at most |F_j| results
        out_ids.fill_(-1)
        out_scores.fill_(float("nan"))
        shared = [j for j in range(b) if n_allowed[j] >= c]
        if shared:
            idx = torch.tensor(shared, dtype=torch.int64, device=corpus.device)
            pid_s, q_s = probe_ids[idx].contiguous(), q_dev[idx].contiguous()
            o_ids, o_sc = default_outputs(len(shared), k, corpus.device)
            u_s, a_s, stride = self._prepare_probe(pid_s, len(shared), npb)
            groups(q_s, u_s, a_s, stride, k, c, o_ids, o_sc)
            out_ids.index_copy_(0, idx, o_ids)
            out_scores.index_copy_(0, idx, o_sc)
        for j in short:
            if n_allowed[j] == 0:
                continue
            kk = min(k, n_allowed[j])
            u_1, a_1, stride = self._prepare_probe(probe_ids[j:j + 1], 1, npb)
            o_ids, o_sc = default_outputs(1, kk, corpus.device)
            # (the cut of a short list: |F_j| on the int8 codes, whose entry point takes no cut above the list; the fp32
            # entry point caps the batch's cut at the list itself)
            groups(q_dev[j:j + 1], u_1, a_1, stride, kk, min(c, n_allowed[j]) if use_i8 else c, o_ids, o_sc)
            out_ids[j, :kk] = o_ids[0]
            out_scores[j, :kk] = o_sc[0]
        return out_ids, out_scores

    # ---------------------------------------------------------------- probe under a user filter
    def _check_probe_filtered(self, k, candidates: Optional[int], similarity: str, filter, nprobe: Optional[int],
                              approx: bool) -> None:
        """The argument errors of ``search_probe_filtered*`` that need no device (raised before anything is built)."""
        from . import _native as nat
        if filter is None:
            raise ValueError("search_probe_filtered needs a filter (search / search_batch are the unfiltered probe)")
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"nprobe must be at least 1, got {nprobe}")
        if approx:
            if not self._int8_codes:
                raise ValueError("approx=True needs an IVFIndex built with int8_codes=True")
            if similarity != "ip":
                raise ValueError("approx=True does not take a similarity transform")
            cut = 2 * int(k) if candidates is None else int(candidates)
            if cut > nat.I8_MAX_CANDIDATES:
                raise ValueError(f"approx=True re-ranks at most {nat.I8_MAX_CANDIDATES} candidates, got a cut of {cut}")

    def _allow_of(self, filter, b: int):
        """``filter`` as the stage reads it -> (device bytes, per-query flag); a stale filter raises ``ValueError``."""
        from ._engine import DeviceQueryFilters
        f = self._prepared(filter)
        if isinstance(f, DeviceQueryFilters):
            self._corpus.check_query_filters(f, b)
            return f.masks, 1
        self._corpus.check_filter(f)
        return f.byte_mask(), 0

    def _prepare_probe_filtered(self, probe_ids, b: int, nprobe: int, allow, per_query: int):
        """``dewi_ivf_probe_prepare_filtered`` into the index's probe buffer -> (|U| per group, |F_j| per query, bytes per
        group): ``_prepare_probe`` with the rows ``allow`` does not hold dropped on the device."""
        import torch
        from . import _native as nat
        lib, st, corpus = nat.load_library(), self._ivf, self._corpus
        need = int(lib.dewi_ivf_probe_filtered_bytes(corpus.n_rows, self.dim, 0, b, PROBE_GROUP))
        stride = int(lib.dewi_ivf_probe_filtered_group_bytes(corpus.n_rows, self.dim, 0, PROBE_GROUP))
        if need == 0 or stride == 0:
            raise nat.NativeLibraryError(f"dewi_ivf_probe_filtered_bytes returned 0 for {b} queries")
        if self._probe_buf is None or self._probe_buf.numel() < need or self._probe_buf.device != corpus.device:
            self._probe_buf = torch.empty(need, dtype=torch.uint8, device=corpus.device)
        n_groups = (b + PROBE_GROUP - 1) // PROBE_GROUP
        n_union = (ctypes.c_int64 * n_groups)()
        n_allowed = (ctypes.c_int64 * b)()
        nat.check(lib.dewi_ivf_probe_prepare_filtered(
            0, corpus.n_rows, self.dim, nat.ptr(st.lists), st.nlist, nat.ptr(probe_ids), b, nprobe, PROBE_GROUP, nat.ptr(allow),
            per_query, nat.ptr(self._probe_buf), self._probe_buf.numel(), n_union, n_allowed, nat.stream_ptr()))
        return list(n_union), list(n_allowed), stride

    def search_probe_filtered_device(self, q_dev, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                                     candidates: Optional[int] = None, similarity: str = "ip", *, filter,
                                     nprobe: Optional[int] = None, widen: bool = False, approx: bool = False,
                                     rescore: bool = True, return_nprobe: bool = False):
        """``search_device`` where query j searches the rows of its ``nprobe`` nearest cells that ``filter`` allows: the three
        steps, with ``dewi_ivf_probe_prepare_filtered`` as step 2 -> (ids int64 [B, k], scores fp32 [B, k]) device tensors, and
        with ``return_nprobe`` the ``nprobe`` every query ended at (int64 [B], on the device).  ``filter``: a ``DeviceFilter``,
        ``DeviceQueryFilters`` or anything ``search_batch(filter=)`` prepares on the fly.  The rules of ``search_device``: groups
        of 8 share a pass, a query with ``|F_j|`` below the cut is searched on its own list with cut ``|F_j|``, ``|F_j| < k`` pads
        with id -1 / score NaN.  Synchronises the stream once per prepared buffer.  See ``search_probe_filtered_batch``."""
        import torch
        from . import _native as nat
        from ._engine import check_search_args, cut_size, default_outputs, empty_result
        approx = bool(approx)
        self._check_probe_filtered(k, candidates, similarity, filter, nprobe, approx)
        self._ensure_built()
        corpus, st = self._corpus, self._ivf
        if corpus.is_bf16:
            raise NotImplementedError("IVFIndex serves fp32 corpora (bf16: not in this build)")
        npb = self._resolve_nprobe(nprobe, st.nlist)
        b, k = check_search_args(q_dev.shape, self.dim, k, candidates, similarity)
        allow, per_query = self._allow_of(filter, b)
        used = [npb] * b                             # the nprobe every query ended at

        def result(ids, scores):
            if not return_nprobe:
                return ids, scores
            return ids, scores, torch.tensor(used, dtype=torch.int64, device=corpus.device)

        if k <= 0:
            return result(*empty_result(b, corpus.device))
        if candidates is not None and int(candidates) < k:
            raise ValueError(f"candidates = {candidates} must be at least k = {k}")
        c = cut_size(k, candidates)
        sim, eta, pref = nat.SIM_CODES[similarity], float(eta), float(entropy_pref)
        out_ids, out_scores = default_outputs(b, k, corpus.device)

        def groups(q, n_union, n_allowed, stride, kk, cc, o_ids, o_sc):
            if approx:
                self._search_groups_i8(q, n_union, n_allowed, stride, kk, cc, rescore, eta, pref, o_ids, o_sc)
            else:
                self._search_groups(q, n_union, n_allowed, stride, kk, cc, candidates, sim, eta, pref, o_ids, o_sc)

        pending = list(range(b))
        while pending:
            # the coarse step runs for the whole batch (nlist rows: cheap), so that a query's cells at a given nprobe never
            # depend on which other queries are still pending
            probe_all, _ = st.coarse.search_device(q_dev, npb, 0.0, 0.0, candidates=npb)
            n_p = len(pending)
            if n_p == b:
                pid, q_p, allow_p = probe_all, q_dev, allow
            else:
                at = torch.tensor(pending, dtype=torch.int64, device=corpus.device)
                pid, q_p = probe_all[at].contiguous(), q_dev[at].contiguous()
                allow_p = allow[at].contiguous() if per_query else allow
            for j in pending:
                used[j] = npb
            n_union, n_allowed, stride = self._prepare_probe_filtered(pid, n_p, npb, allow_p, per_query)
            ready = [i for i in range(n_p) if n_allowed[i] >= c]
            if len(ready) == b:                      # the usual case: every list reaches the cut at the first probe
                groups(q_dev, n_union, n_allowed, stride, k, c, out_ids, out_scores)
                return result(out_ids, out_scores)
            if n_p == b:                             # somebody is short: rows are written one by one, the rest is padding
                out_ids.fill_(-1)
                out_scores.fill_(float("nan"))
            again = [i for i in range(n_p) if n_allowed[i] < c] if widen and npb < st.nlist else []
            short = [i for i in range(n_p) if 0 < n_allowed[i] < c and i not in again]
            if ready:
                o_ids, o_sc = default_outputs(len(ready), k, corpus.device)
                if len(ready) == n_p:
                    groups(q_p, n_union, n_allowed, stride, k, c, o_ids, o_sc)
                else:                                # the lists that reach the cut, prepared again as a batch of their own
                    sub = torch.tensor(ready, dtype=torch.int64, device=corpus.device)
                    pid_s, q_s = pid[sub].contiguous(), q_p[sub].contiguous()
                    allow_s = allow_p[sub].contiguous() if per_query else allow_p
                    u_s, a_s, stride = self._prepare_probe_filtered(pid_s, len(ready), npb, allow_s, per_query)
                    groups(q_s, u_s, a_s, stride, k, c, o_ids, o_sc)
                dst = torch.tensor([pending[i] for i in ready], dtype=torch.int64, device=corpus.device)
                out_ids.index_copy_(0, dst, o_ids)
                out_scores.index_copy_(0, dst, o_sc)
            for i in short:                          # one list each, cut and k limited to |F_j|
                j, kk = pending[i], min(k, n_allowed[i])
                allow_1 = allow_p[i:i + 1] if per_query else allow_p
                u_1, a_1, stride = self._prepare_probe_filtered(pid[i:i + 1], 1, npb, allow_1, per_query)
                o_ids, o_sc = default_outputs(1, kk, corpus.device)
                groups(q_p[i:i + 1], u_1, a_1, stride, kk, min(c, n_allowed[i]) if approx else c, o_ids, o_sc)
                out_ids[j, :kk] = o_ids[0]
                out_scores[j, :kk] = o_sc[0]
            pending = [pending[i] for i in again]
            npb = min(2 * npb, st.nlist)
        return result(out_ids, out_scores)

    def search_probe_filtered_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                                    candidates: Optional[int] = None, similarity: str = "ip", *, filter,
                                    nprobe: Optional[int] = None, widen: bool = False, approx: bool = False,
                                    rescore: bool = True, return_nprobe: bool = False):
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k][, nprobe_used int64 [B]]): the probe of
        ``search_batch`` UNDER a user filter.  Query j's answer is, bit for bit, ``ExactIndex.search_batch(q_j, k', ...,
        filter=<rows of its probed cells that its allow-list holds>)``; the cells are expanded and filtered on the device
        (``dewi_ivf_probe_prepare_filtered``: work proportional to the probed rows, not to N).

        ``filter`` (required; ``None`` raises ``ValueError``): whatever ``ExactIndex.search_batch(filter=)`` takes — a bool
        mask, doc ids, rows, a prepared ``DeviceFilter``, ``dedup_filter(...)``, or per query a bool [B, N] mask /
        ``DeviceQueryFilters``.  A stale filter raises ``ValueError``.  Short lists do not raise: ``|F_j| < k`` pads the row
        with id -1 / score NaN, ``|F_j| = 0`` is an all-padded row.

        ``widen=True``: a query whose ``|F_j|`` is below the cut is probed again with ``nprobe`` doubled (capped at ``nlist``)
        until it reaches the cut or ``nprobe == nlist`` (there the answer is the exact filtered search); its answer is the
        rule above at its final ``nprobe_j``, which ``return_nprobe=True`` returns.  Only the short queries are re-run.

        ``approx=True`` (an index with ``int8_codes=True``, ``similarity="ip"``, a cut of at most 1024; else ``ValueError``):
        the cut is taken by the int8 scores — query j's answer is ``search_approx_filtered`` on the same rows; ``rescore``
        as there.  ``approx=False`` is the default: nothing about this combination has been measured to choose by."""
        self._check_probe_filtered(k, candidates, similarity, filter, nprobe, bool(approx))
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        import torch
        corpus = self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            q_dev = corpus.stage_queries(q)
            out = self.search_probe_filtered_device(q_dev, k, eta, entropy_pref, candidates, similarity, filter=filter,
                                                    nprobe=nprobe, widen=widen, approx=approx, rescore=bool(rescore),
                                                    return_nprobe=return_nprobe)
            return tuple(t.cpu().numpy() for t in out)

    def search_probe_filtered(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                              candidates: Optional[int] = None, similarity: str = "ip", *, filter,
                              nprobe: Optional[int] = None, widen: bool = False, approx: bool = False, rescore: bool = True,
                              return_nprobe: bool = False):
        """``search_probe_filtered_batch`` for one query -> ``SearchResult`` (fewer than k results when the probed cells hold
        fewer than k allowed rows), with ``return_nprobe`` the pair (``SearchResult``, nprobe used)."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        out = self.search_probe_filtered_batch(q[:1], k, eta, entropy_pref, candidates, similarity, filter=filter,
                                               nprobe=nprobe, widen=widen, approx=approx, rescore=rescore,
                                               return_nprobe=return_nprobe)
        keep = out[0][0] >= 0
        result = self.results_for(out[0][:1][:, keep], out[1][:1][:, keep])[0]
        return (result, int(out[2][0])) if return_nprobe else result

    def search_batch(self, queries: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
                     candidates: Optional[int] = None, similarity: str = "ip", *, approx: Optional[bool] = None,
                     rescore: bool = True, filter=None, nprobe: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """[B, dim] queries -> (row indices int64 [B, k], adjusted scores fp32 [B, k]); query j searches the rows F_j of its
        ``nprobe`` nearest cells with the rules of ``ExactIndex.search`` on those rows (cut ``min(2k, |F_j|)`` or
        ``candidates``, blend, top-k).  An approximate index does not raise when the probe is short: with ``|F_j| < k`` the
        row holds ``|F_j|`` results and is padded with id -1 / score NaN.

        ``filter=`` here runs the parent's EXACT filtered search over the whole allow-list (``nprobe`` is then ignored);
        the probe under a filter is ``search_probe_filtered_batch``.

        ``approx`` (an index made with ``int8_codes=True``): step 3 takes the cut of every query by the INT8 scores of its
        probed rows (a quarter of the bytes), re-scores it from the fp32 rows (``rescore=True``; ``False`` blends the int8
        scores as they are) and finishes with the same blend — query j's answer is ``search_approx_filtered`` on the rows of
        its cells.  ``None`` (default): taken iff the index has codes, ``similarity == "ip"``, there is no ``filter``, the
        cut is at most 1024 and the batch at most ``APPROX_AUTO_MAX_BATCH``; ``False``: the fp32 probe, bit for bit;
        ``True`` without codes, with a ``filter`` or a transform raises ``ValueError``."""
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"nprobe must be at least 1, got {nprobe}")
        use_i8 = self._use_approx_probe(approx, similarity, filter, k, candidates,      # (argument errors before any build)
                                        np.shape(queries)[0] if np.ndim(queries) == 2 else 1)
        if filter is not None:
            return super().search_batch(queries, k, eta, entropy_pref, candidates, similarity, filter=filter)
        self._ensure_built()
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        import torch
        corpus = self._corpus
        with corpus._lock, torch.cuda.device(corpus.device):
            q_dev = corpus.stage_queries(q)
            ids, scores = self.search_device(q_dev, k, eta, entropy_pref, candidates, similarity, nprobe, approx=use_i8,
                                             rescore=bool(rescore))
            return ids.cpu().numpy(), scores.cpu().numpy()

    def search(self, query: np.ndarray, k: int = 10, eta: float = 0.5, entropy_pref: float = 0.0,
               candidates: Optional[int] = None, similarity: str = "ip", *, approx: Optional[bool] = None,
               rescore: bool = True, filter=None, nprobe: Optional[int] = None) -> SearchResult:
        """``ExactIndex.search`` over the rows of the query's ``nprobe`` nearest cells (see ``search_batch``); fewer than k
        results when those cells hold fewer than k rows."""
        q = np.asarray(query, dtype=np.float32)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        rows, scores = self.search_batch(q, k, eta, entropy_pref, candidates, similarity, approx=approx, rescore=rescore,
                                         filter=filter, nprobe=nprobe)
        keep = rows[0] >= 0
        return self.results_for(rows[:1][:, keep], scores[:1][:, keep])[0]

    # ---------------------------------------------------------------- persistence
    def save(self, path: Union[str, Path]) -> None:
        """The ``ExactIndex`` files unchanged (the directory still loads as an ``ExactIndex``) plus ``ivf.json``,
        ``ivf_centroids.npy`` and ``ivf_assign.npy``."""
        self._ensure_built()
        super().save(path)
        root = Path(path)
        st = self._ivf
        with open(root / "ivf.json", "w") as fh:
            json.dump({"format_version": IVF_FORMAT_VERSION, "nlist": st.nlist, "nprobe": self.nprobe,
                       "train_seed": self.train_seed, "train_iters": self.train_iters, "max_train_rows": self.max_train_rows,
                       "num_rows": int(self._corpus.n_rows)}, fh)
        np.save(str(root / "ivf_centroids.npy"), st.centroids.cpu().numpy())
        np.save(str(root / "ivf_assign.npy"), st.assign.cpu().numpy())

    @classmethod
    def load(cls, path: Union[str, Path], **kwargs: Any) -> "IVFIndex":
        """Load without retraining: the saved centroids and assignment are taken as they are (a directory without the IVF
        files — one an ``ExactIndex`` saved — loads too and is trained at the first build)."""
        root = Path(path)
        meta = None
        if (root / "ivf.json").exists():
            with open(root / "ivf.json") as fh:
                meta = json.load(fh)
            if meta.get("format_version") != IVF_FORMAT_VERSION:
                raise ValueError(f"unknown ivf.json format version {meta.get('format_version')}")
            for key in ("nlist", "nprobe", "train_seed", "train_iters", "max_train_rows"):
                kwargs.setdefault(key, meta[key])
        inst = super().load(path, **kwargs)
        if meta is not None:
            inst._ivf_loaded = (np.load(str(root / "ivf_centroids.npy"), allow_pickle=False),
                                np.load(str(root / "ivf_assign.npy"), allow_pickle=False))
        return inst

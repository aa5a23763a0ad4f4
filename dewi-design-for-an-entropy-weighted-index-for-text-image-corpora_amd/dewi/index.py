"""``DewiIndex`` — the façade users construct (reference ``src/dewi/index.py``).

Same constructor, defaults and methods as the reference (index.py:22-166): it validates
the query, fills in the default ``eta`` / ``entropy_pref`` and delegates to a backend.  In
this build every backend choice resolves to the HIP ``ExactIndex`` (ANN graph libraries
are out of scope), with the reference's own warning when an ANN backend was asked for.
Additions: ``add_batch``, ``search_batch``, ``range_search``, ``range_search_batch``, ``near_duplicates``, ``duplicate_groups``,
``dedup_filter``, ``make_groups`` / ``search_collapsed`` / ``search_collapsed_batch``, ``search_by_examples`` and the in-place ``remove`` / ``upsert`` / ``upsert_batch`` / ``upsert_batch_columns`` / ``rows_of`` / ``reserve``.
Attribute columns and predicates over them (``set_attributes``, ``attributes_from_payload``, ``update_attributes``,
``attributes_of``, ``make_filter_where``, ``make_query_filters_where``, ``count_where``; ``filter=`` takes a ``dewi.where.Where``).
"""
from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import backends as _backends
from .backends import (BaseIndex, ExactIndex, FAISSIndex, HNSWIndex, IndexBackend, _HAS_FAISS, _HAS_HNSW)
from .types import Payload

logger = logging.getLogger(__name__)


class DewiIndex(BaseIndex):
    def __init__(self, dim: int, space: str = "cosine", backend: Union[str, IndexBackend] = "auto", ef: int = 200,
                 M: int = 32, use_ann: bool = True, ef_query: int = 200, rerank_eta: float = 0.25,
                 entropy_pref: float = 0.0, **kwargs: Any):
        super().__init__(dim, space)
        self._meta: Dict[str, Dict[str, Any]] = {}
        self.ef_query = ef_query
        self.rerank_eta = float(rerank_eta)
        self.entropy_pref = float(entropy_pref)
        self._built = False
        self._use_ann = bool(use_ann)
        if isinstance(backend, str):
            try:
                backend = IndexBackend.from_str(backend)
            except KeyError:
                backend = IndexBackend.EXACT          # unknown names fall back (index.py:44-48)
        self._requested_backend = backend
        if self._use_ann and backend is not IndexBackend.EXACT:
            # index.py:58-60: requested ANN library missing -> warn, use the exact index
            logger.warning("ANN backend unavailable; falling back to ExactIndex.")
        # (additive switches of the exact backend; everything else in **kwargs is accepted and ignored as in the reference)
        exact_kwargs = {k: v for k, v in kwargs.items() if k in ("device", "batch_shadow", "shadow_single_query", "int8_shadow", "binary_shadow")}
        self._backend: BaseIndex = ExactIndex(dim, space, **exact_kwargs)

    # ------------------------------------------------------------------ ingest / build
    def add(self, doc_id: str, embedding: np.ndarray, payload: Payload, meta: Optional[Dict[str, Any]] = None) -> None:
        if meta is not None:
            self._meta[doc_id] = meta
        self._backend.add(doc_id, np.asarray(embedding, dtype=np.float32), payload)
        self._built = False

    def add_batch(self, doc_ids: Sequence[str], embeddings: np.ndarray, payloads: Sequence[Payload]) -> None:
        self._backend.add_batch(doc_ids, np.asarray(embeddings, dtype=np.float32), payloads)
        self._built = False

    def add_batch_columns(self, doc_ids: Sequence[str], embeddings: np.ndarray, columns: Dict[str, np.ndarray]) -> None:
        """Bulk ingest with the payloads as one float array per ``Payload`` field (no object per row)."""
        self._backend.add_batch_columns(doc_ids, embeddings, columns)
        self._built = False

    def build(self) -> None:
        self._backend.build()
        self._built = True

    # ------------------------------------------------------------------ remove / upsert in place (additive)
    def remove(self, doc_ids: Sequence[str]) -> int:
        """Delete documents from the built index in place (``ExactIndex.remove``): no rebuild; the metadata goes too, and
        ``get_payload`` / ``get_embedding`` / ``get_metadata`` of a removed id return ``None``."""
        ids = [doc_ids] if isinstance(doc_ids, str) else list(doc_ids)
        n = self._backend.remove(ids)
        for d in ids:
            self._meta.pop(d, None)
        self._built = True
        return n

    def upsert(self, doc_id: str, embedding: np.ndarray, payload: Payload, meta: Optional[Dict[str, Any]] = None) -> None:
        """Replace ``doc_id``'s embedding and payload in place, or append it (``ExactIndex.upsert``); ``meta`` sets its
        metadata."""
        self._backend.upsert(doc_id, np.asarray(embedding, dtype=np.float32), payload)
        if meta is not None:
            self._meta[doc_id] = meta
        self._built = True

    def upsert_batch(self, doc_ids: Sequence[str], embeddings: np.ndarray, payloads: Sequence[Payload]) -> Tuple[int, int]:
        out = self._backend.upsert_batch(doc_ids, np.asarray(embeddings, dtype=np.float32), payloads)
        self._built = True
        return out

    def upsert_batch_columns(self, doc_ids: Sequence[str], embeddings, columns: Dict[str, np.ndarray]) -> Tuple[int, int]:
        out = self._backend.upsert_batch_columns(doc_ids, embeddings, columns)
        self._built = True
        return out

    def rows_of(self, doc_ids: Sequence[str]) -> np.ndarray:
        return self._backend.rows_of(doc_ids)

    def reserve(self, rows: int) -> None:
        self._backend.reserve(rows)
        self._built = True

    @property
    def capacity(self) -> int:
        return self._backend.capacity

    # ------------------------------------------------------------------ search (A5)
    def _defaults(self, eta: Optional[float], entropy_pref: Optional[float]) -> Tuple[float, float]:
        return (self.rerank_eta if eta is None else eta, self.entropy_pref if entropy_pref is None else entropy_pref)

    def make_filter(self, mask=None, *, doc_ids: Optional[Sequence[str]] = None, rows=None):
        """Prepare an allow-list for ``search`` / ``search_batch(filter=...)`` (``ExactIndex.make_filter``)."""
        if not self._built:
            self.build()
        return self._backend.make_filter(mask, doc_ids=doc_ids, rows=rows)

    def make_query_filters(self, masks=None, *, doc_ids=None, rows=None):
        """Prepare one allow-list per query for ``search_batch(filter=...)`` (``ExactIndex.make_query_filters``)."""
        if not self._built:
            self.build()
        return self._backend.make_query_filters(masks, doc_ids=doc_ids, rows=rows)

    def _approx_kwargs(self, approx: Optional[bool], rescore: bool) -> Dict[str, Any]:
        """The int8 route's keywords for the backend: nothing for a call that leaves them at their defaults (the backend then
        sees exactly the call it always saw)."""
        return {} if approx is None and rescore else {"approx": approx, "rescore": rescore}

    def search(self, query: np.ndarray, k: int = 10, eta: Optional[float] = None,
               entropy_pref: Optional[float] = None, *, approx: Optional[bool] = None, rescore: bool = True,
               filter=None) -> List[Tuple[str, float, Payload]]:
        """``filter`` (additive): search only an allow-list — a prepared filter (``make_filter``), a bool mask, doc ids
        or row positions.  ``approx`` / ``rescore`` (additive; an index made with ``int8_shadow=True``): the approximate
        int8 route of ``ExactIndex.search_batch`` — ``None``: taken where the index has an int8 shadow; ``True`` without
        one, or together with ``filter``, raises ``ValueError``; ``False``: the exact path."""
        if not self._built:
            self.build()
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        if filter is not None:
            return self._backend.search(q, k, eta, entropy_pref, filter=filter, **self._approx_kwargs(approx, rescore))
        return self._backend.search(q, k, eta, entropy_pref, **self._approx_kwargs(approx, rescore))

    def search_batch(self, queries: np.ndarray, k: int = 10, eta: Optional[float] = None,
                     entropy_pref: Optional[float] = None, *, approx: Optional[bool] = None, rescore: bool = True,
                     filter=None) -> List[List[Tuple[str, float, Payload]]]:
        """One call for B queries ([B, dim]); each result list equals ``search`` of that row (``filter``, ``approx``,
        ``rescore``: see ``search``; per-query filters — ``make_query_filters`` or a bool [B, N] mask — give ``[]`` for a
        query whose list is empty)."""
        if not self._built:
            self.build()
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if filter is not None:
            rows, scores = self._backend.search_batch(q, k, eta, entropy_pref, filter=filter,
                                                      **self._approx_kwargs(approx, rescore))
            if rows.size and (rows < 0).any():     # per-query filters: an empty list pads its row with id -1
                n_real = (rows >= 0).sum(axis=1)
                res = self._backend.results_for(np.where(rows < 0, 0, rows), scores)
                return [r[:int(m)] for r, m in zip(res, n_real)]
        else:
            rows, scores = self._backend.search_batch(q, k, eta, entropy_pref, **self._approx_kwargs(approx, rescore))
        return self._backend.results_for(rows, scores)

    def search_by_examples(self, positive, negative=None, k: int = 10, eta: Optional[float] = None,
                           entropy_pref: Optional[float] = None, *, match: str = "any", negative_rule: str = "penalty",
                           negative_weight: float = 1.0, candidates: Optional[int] = None, filter=None,
                           exclude_examples: bool = True) -> List[Tuple[str, float, Payload]]:
        """Search by examples (additive; ``ExactIndex.search_by_examples``): ``positive`` / ``negative`` are doc ids and / or
        ``[dim]`` vectors, at most 16 together; every document is scored by its nearest (``match="any"``) or farthest
        (``"all"``) positive, less what ``negative_rule`` takes off for its nearest negative."""
        if not self._built:
            self.build()
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        return self._backend.search_by_examples(positive, negative, k, eta, entropy_pref, match=match,
                                                negative_rule=negative_rule, negative_weight=negative_weight,
                                                candidates=candidates, filter=filter, exclude_examples=exclude_examples)

    def search_binary(self, query: np.ndarray, k: int = 10, eta: Optional[float] = None, entropy_pref: Optional[float] = None,
                      *, candidates: Optional[int] = None, rescore: bool = True) -> List[Tuple[str, float, Payload]]:
        """``search`` with the candidate cut taken by Hamming distance over the 1-bit copy of the rows
        (``ExactIndex.search_binary_batch``; an index made with ``binary_shadow=True``)."""
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        return self.search_binary_batch(q.reshape(1, -1), k, eta, entropy_pref, candidates=candidates, rescore=rescore)[0]

    def search_binary_batch(self, queries: np.ndarray, k: int = 10, eta: Optional[float] = None,
                            entropy_pref: Optional[float] = None, *, candidates: Optional[int] = None,
                            rescore: bool = True) -> List[List[Tuple[str, float, Payload]]]:
        """One call for B queries ([B, dim]); each result list equals ``search_binary`` of that row."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if not getattr(self._backend, "_binary_shadow", False):         # (argument errors before any build)
            raise ValueError("search_binary needs an index built with binary_shadow=True")
        if not self._built:
            self.build()
        rows, scores = self._backend.search_binary_batch(q, k, eta, entropy_pref, candidates=candidates, rescore=rescore)
        return self._backend.results_for(rows, scores)

    def search_approx_filtered(self, query: np.ndarray, k: int = 10, eta: Optional[float] = None,
                               entropy_pref: Optional[float] = None, candidates: Optional[int] = None, *, filter,
                               rescore: bool = True) -> List[Tuple[str, float, Payload]]:
        """``search(filter=...)`` with the candidate cut taken by the int8 scores of the allowed rows
        (``ExactIndex.search_approx_filtered_batch``; an index made with ``int8_shadow=True``)."""
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        return self.search_approx_filtered_batch(q.reshape(1, -1), k, eta, entropy_pref, candidates, filter=filter,
                                                 rescore=rescore)[0]

    def search_approx_filtered_batch(self, queries: np.ndarray, k: int = 10, eta: Optional[float] = None,
                                     entropy_pref: Optional[float] = None, candidates: Optional[int] = None, *, filter,
                                     rescore: bool = True) -> List[List[Tuple[str, float, Payload]]]:
        """One call for B queries ([B, dim]); each result list equals ``search_approx_filtered`` of that row (per-query
        filters give ``[]`` for a query whose list is empty)."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if not getattr(self._backend, "_int8_shadow", False):          # (argument errors before any build)
            raise ValueError("search_approx_filtered needs an index built with int8_shadow=True")
        if not self._built:
            self.build()
        rows, scores = self._backend.search_approx_filtered_batch(q, k, eta, entropy_pref, candidates, filter=filter,
                                                                  rescore=rescore)
        n_real = (rows >= 0).sum(axis=1)
        res = self._backend.results_for(np.where(rows < 0, 0, rows), scores)
        return [r[:int(m)] for r, m in zip(res, n_real)]

    def search_diverse_approx(self, query: np.ndarray, k: int = 10, eta: Optional[float] = None,
                              entropy_pref: Optional[float] = None, mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                              max_sim: Optional[float] = None, rescore: bool = True) -> List[Tuple[str, float, Payload]]:
        """``search_diverse`` over the pool the int8 route picks (``ExactIndex.search_diverse_approx``; an index made with
        ``int8_shadow=True``)."""
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        return self.search_diverse_approx_batch(q.reshape(1, -1), k, eta, entropy_pref, mmr_lambda, candidates, max_sim,
                                                rescore)[0]

    def search_diverse_approx_batch(self, queries: np.ndarray, k: int = 10, eta: Optional[float] = None,
                                    entropy_pref: Optional[float] = None, mmr_lambda: float = 0.5,
                                    candidates: Optional[int] = None, max_sim: Optional[float] = None,
                                    rescore: bool = True) -> List[List[Tuple[str, float, Payload]]]:
        """One call for B queries ([B, dim]); each result list equals ``search_diverse_approx`` of that row."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if not self._built:
            self.build()
        rows, scores = self._backend.search_diverse_approx_batch(q, k, eta, entropy_pref, mmr_lambda, candidates, max_sim,
                                                                 rescore)
        n_real = (rows >= 0).sum(axis=1)
        res = self._backend.results_for(np.where(rows < 0, 0, rows), scores)
        return [r[:int(m)] for r, m in zip(res, n_real)]

    def search_diverse(self, query: np.ndarray, k: int = 10, eta: Optional[float] = None,
                       entropy_pref: Optional[float] = None, mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                       max_sim: Optional[float] = None) -> List[Tuple[str, float, Payload]]:
        """``search`` re-ranked for diversity (additive; ``ExactIndex.search_diverse``): maximal marginal relevance over
        the ``candidates`` most similar documents (default ``4k``), results in pick order, possibly fewer than k when
        ``max_sim`` strikes candidates out."""
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        return self.search_diverse_batch(q.reshape(1, -1), k, eta, entropy_pref, mmr_lambda, candidates, max_sim)[0]

    def search_diverse_batch(self, queries: np.ndarray, k: int = 10, eta: Optional[float] = None,
                             entropy_pref: Optional[float] = None, mmr_lambda: float = 0.5, candidates: Optional[int] = None,
                             max_sim: Optional[float] = None) -> List[List[Tuple[str, float, Payload]]]:
        """One call for B queries ([B, dim]); each result list equals ``search_diverse`` of that row."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if self.space == "l2":
            raise NotImplementedError("diverse search penalises the inner product of unit rows: space='l2' is not in this build")
        if not self._built:
            self.build()
        rows, scores = self._backend.search_diverse_batch(q, k, eta, entropy_pref, mmr_lambda, candidates, max_sim)
        n_real = (rows >= 0).sum(axis=1)           # fewer than k eligible documents: the tail is padded with id -1
        res = self._backend.results_for(np.where(rows < 0, 0, rows), scores)
        return [r[:int(m)] for r, m in zip(res, n_real)]

    def select_subset(self, budget: int, mmr_lambda: float = 0.5, max_sim: Optional[float] = None, relevance=None,
                      filter=None, seeds=None, return_gain: bool = False, return_coverage: bool = False):
        """The ``budget`` most informative documents that do not repeat each other (additive; ``ExactIndex.select_subset``):
        greedy DEWI-weighted coverage of the whole corpus, doc ids in pick order."""
        if self.space == "l2":
            raise NotImplementedError("subset selection penalises the inner product of unit rows: space='l2' is not in this build")
        if not self._built:
            self.build()
        return self._backend.select_subset(budget, mmr_lambda, max_sim, relevance, filter, seeds, return_gain, return_coverage)

    def select_subset_blocked(self, budget: int, mmr_lambda: float = 0.5, max_sim: Optional[float] = None, relevance=None,
                              filter=None, seeds=None, return_gain: bool = False, return_coverage: bool = False,
                              picks_per_pass: Optional[int] = 32):
        """``select_subset`` with up to ``picks_per_pass`` picks per corpus pass, the same answer bit for bit (additive;
        ``ExactIndex.select_subset_blocked``)."""
        if self.space == "l2":
            raise NotImplementedError("subset selection penalises the inner product of unit rows: space='l2' is not in this build")
        if not self._built:
            self.build()
        return self._backend.select_subset_blocked(budget, mmr_lambda, max_sim, relevance, filter, seeds, return_gain,
                                                   return_coverage, picks_per_pass)

    def select_subset_grouped(self, budget: int, *, groups, per_group: int = 1, quotas=None, mmr_lambda: float = 0.5,
                              max_sim: Optional[float] = None, relevance=None, filter=None, seeds=None, seeds_count: bool = True,
                              return_gain: bool = False, return_coverage: bool = False, picks_per_pass: Optional[int] = 32):
        """``select_subset`` with at most ``per_group`` picks from one group of ``groups`` (additive;
        ``ExactIndex.select_subset_grouped``)."""
        if self.space == "l2":
            raise NotImplementedError("subset selection penalises the inner product of unit rows: space='l2' is not in this build")
        if not self._built:
            self.build()
        return self._backend.select_subset_grouped(budget, groups=groups, per_group=per_group, quotas=quotas, mmr_lambda=mmr_lambda,
                                                   max_sim=max_sim, relevance=relevance, filter=filter, seeds=seeds,
                                                   seeds_count=seeds_count, return_gain=return_gain,
                                                   return_coverage=return_coverage, picks_per_pass=picks_per_pass)

    def make_groups(self, groups):
        """Prepare group labels for ``search_collapsed`` / ``search_collapsed_batch`` (``ExactIndex.make_groups``)."""
        if not self._built:
            self.build()
        return self._backend.make_groups(groups)

    def search_collapsed(self, query: np.ndarray, k: int = 10, eta: Optional[float] = None,
                         entropy_pref: Optional[float] = None, *, groups, per_group: int = 1, candidates: Optional[int] = None,
                         filter=None, approx: bool = False, rescore: bool = True, widen: bool = False,
                         return_hits: bool = False):
        """``search`` with at most ``per_group`` results from one group of ``groups`` (additive;
        ``ExactIndex.search_collapsed``): possibly fewer than k results; with ``return_hits=True`` ``(results, hits)``."""
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        out = self.search_collapsed_batch(q.reshape(1, -1), k, eta, entropy_pref, groups=groups, per_group=per_group,
                                          candidates=candidates, filter=filter, approx=approx, rescore=rescore, widen=widen,
                                          return_hits=return_hits)
        return (out[0][0], out[1][0]) if return_hits else out[0]

    def search_collapsed_batch(self, queries: np.ndarray, k: int = 10, eta: Optional[float] = None,
                               entropy_pref: Optional[float] = None, *, groups, per_group: int = 1,
                               candidates: Optional[int] = None, filter=None, approx: bool = False, rescore: bool = True,
                               widen: bool = False, return_hits: bool = False):
        """One call for B queries ([B, dim]); each result list equals ``search_collapsed`` of that row.  With
        ``return_hits=True``: ``(results, hits)``, ``hits[j]`` the list of group sizes in the pool for query j's results."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        if not self._built:
            self.build()
        rows, scores, hits = self._backend.search_collapsed_batch(q, k, eta, entropy_pref, groups=groups, per_group=per_group,
                                                                  candidates=candidates, filter=filter, approx=approx,
                                                                  rescore=rescore, widen=widen, return_hits=True)
        n_real = (rows >= 0).sum(axis=1)           # fewer than k results: the tail is padded with id -1
        res = self._backend.results_for(np.where(rows < 0, 0, rows), scores)
        res = [r[:int(m)] for r, m in zip(res, n_real)]
        if return_hits:
            return res, [h[:int(m)].tolist() for h, m in zip(hits, n_real)]
        return res

    def range_search(self, query: np.ndarray, threshold: float, eta: Optional[float] = None,
                     entropy_pref: Optional[float] = None, filter=None,
                     max_results: Optional[int] = None) -> List[Tuple[str, float, Payload]]:
        """Every document at least as similar to ``query`` as ``threshold`` (additive; ``ExactIndex.range_search``), in
        ``search`` order; ``[]`` when nothing reaches the threshold or the index is empty."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(query, dtype=np.float32)
        if q.shape != (self.dim,):
            raise ValueError(f"Expected query shape ({self.dim},), got {q.shape}")
        return self.range_search_batch(q.reshape(1, -1), threshold, eta, entropy_pref, filter=filter, max_results=max_results)[0]

    def range_search_batch(self, queries: np.ndarray, threshold, eta: Optional[float] = None,
                           entropy_pref: Optional[float] = None, filter=None,
                           max_results: Optional[int] = None) -> List[List[Tuple[str, float, Payload]]]:
        """One call for B queries ([B, dim]; ``threshold``: one number or one per query); each result list equals
        ``range_search`` of that row."""
        eta, entropy_pref = self._defaults(eta, entropy_pref)
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"Expected queries of shape (B, {self.dim}), got {q.shape}")
        # (the backend checks the arguments, then builds itself on first use; an empty index answers with empty results)
        lims, rows, scores, _ = self._backend.range_search_batch(q, threshold, eta, entropy_pref, filter=filter,
                                                                 max_results=max_results)
        if len(self) > 0 and q.shape[0] > 0:
            self._built = True
        return [self._backend.results_for(rows[None, lims[j]:lims[j + 1]], scores[None, lims[j]:lims[j + 1]])[0]
                for j in range(q.shape[0])]

    def near_duplicates(self, threshold: float, max_pairs: Optional[int] = None, doc_ids: bool = False):
        """Every pair of documents at least ``threshold`` similar (additive; ``ExactIndex.near_duplicates``): rows
        ``(a, b, sims)`` with ``a < b``, or doc-id pairs.  Exact, whatever the backend probes for ``search``."""
        out = self._backend.near_duplicates(threshold, max_pairs=max_pairs, doc_ids=doc_ids)
        if len(self) > 1:
            self._built = True
        return out

    def duplicate_groups(self, threshold: float, keep: str = "dewi", doc_ids: bool = False):
        """The near-duplicate groups (additive; ``ExactIndex.duplicate_groups``): labels, sizes, representatives, the number
        of groups and, with ``doc_ids=True``, the clusters as lists of doc ids.  Exact, whatever the backend probes."""
        out = self._backend.duplicate_groups(threshold, keep=keep, doc_ids=doc_ids)
        if len(self) > 1:
            self._built = True
        return out

    def dedup_filter(self, threshold: float, keep: str = "dewi"):
        """An allow-list of one document per near-duplicate group (additive; ``ExactIndex.dedup_filter``) for
        ``search`` / ``search_batch`` / ``range_search(filter=...)``."""
        out = self._backend.dedup_filter(threshold, keep=keep)
        self._built = True
        return out

    # ------------------------------------------------------------------ attribute columns and predicates (additive)
    def _built_backend(self):
        if not self._built:
            self.build()
        return self._backend

    def set_attributes(self, **columns) -> None:
        """Set per-document attribute columns by name (``ExactIndex.set_attributes``): integers, floats or strings, one
        value per document; ``filter=`` then takes ``dewi.where`` predicates over them."""
        self._built_backend().set_attributes(**columns)

    def attribute_names(self) -> List[str]:
        return self._backend.attribute_names()

    def attribute_schema(self):
        return self._backend.attribute_schema()

    def drop_attributes(self, *names: str) -> None:
        self._built_backend().drop_attributes(*names)

    def attributes_from_payload(self, *fields: str) -> None:
        """Mirror ``Payload`` fields as fp32 attribute columns of the same name (``ExactIndex.attributes_from_payload``)."""
        self._built_backend().attributes_from_payload(*fields)

    def update_attributes(self, doc_ids: Sequence[str], **values) -> None:
        self._built_backend().update_attributes(doc_ids, **values)

    def attributes_of(self, doc_ids: Sequence[str]) -> Dict[str, Any]:
        return self._built_backend().attributes_of(doc_ids)

    def make_filter_where(self, where, base=None):
        """Prepare the allow-list of a ``dewi.where`` predicate on the device (``ExactIndex.make_filter_where``)."""
        return self._built_backend().make_filter_where(where, base=base)

    def make_query_filters_where(self, wheres, base=None):
        """One predicate per query (``ExactIndex.make_query_filters_where``)."""
        return self._built_backend().make_query_filters_where(wheres, base=base)

    def count_where(self, where) -> int:
        return self._built_backend().count_where(where)

    # ------------------------------------------------------------------ facets (additive)
    def facet(self, column, *, filter=None, rows=None, bins=None, value=None):
        """How the selected documents are distributed over an attribute column (``ExactIndex.facet``)."""
        return self._built_backend().facet(column, filter=filter, rows=rows, bins=bins, value=value)

    def facets(self, columns, *, filter=None, rows=None, bins=None, value=None):
        """``facet`` for several columns over the same selections (``ExactIndex.facets``)."""
        return self._built_backend().facets(columns, filter=filter, rows=rows, bins=bins, value=value)

    def facet_range(self, queries, thresholds, column, *, filter=None, value=None, bins=None):
        """One ``Facet`` per query over its range-search results (``ExactIndex.facet_range``)."""
        return self._built_backend().facet_range(queries, thresholds, column, filter=filter, value=value, bins=bins)

    def stratify_by_dewi(self, bins, *, filter=None, rows=None):
        """``{(lo, hi): proportion}`` of the ``dewi`` attribute over the selected documents (``ExactIndex.stratify_by_dewi``)."""
        return self._built_backend().stratify_by_dewi(bins, filter=filter, rows=rows)

    # ------------------------------------------------------------------ accessors (index.py:95-119)
    def __len__(self) -> int:
        return len(self._backend._doc_ids)

    def get_payload(self, doc_id: str) -> Optional[Payload]:
        return self._backend._payloads.get(doc_id)

    def get_embedding(self, doc_id: str) -> Optional[np.ndarray]:
        store = getattr(self._backend, "_embeddings", None)
        if store is None:
            return None
        try:
            return store[self._backend._doc_ids.index(doc_id)]
        except (ValueError, IndexError):
            return None

    def get_metadata(self, doc_id: str) -> Optional[Dict[str, Any]]:
        return self._meta.get(doc_id)

    # ------------------------------------------------------------------ persistence (index.py:121-166)
    def save(self, path: Union[str, Path]) -> None:
        root = Path(path)
        root.mkdir(parents=True, exist_ok=True)
        self._backend.save(root / "ann_index")
        cfg = {"dim": self.dim, "space": self.space, "use_ann": self._use_ann, "ef_query": self.ef_query,
               "rerank_eta": self.rerank_eta, "entropy_pref": self.entropy_pref, "built": self._built,
               "backend_type": type(self._backend).__name__}
        with open(root / "config.json", "w", encoding="utf-8") as fh:
            json.dump(cfg, fh)
        if self._meta:
            with open(root / "meta.json", "w", encoding="utf-8") as fh:
                json.dump(self._meta, fh)

    @classmethod
    def load(cls, path: Union[str, Path], **kwargs: Any) -> "DewiIndex":
        """``kwargs`` (additive): the exact backend's switches, e.g. ``int8_shadow=True`` or ``binary_shadow=True`` — nothing of
        either copy is on disk; it is made again from the fp32 rows at the first build, and both codes are deterministic, so a
        loaded index answers bit-equally."""
        root = Path(path)
        with open(root / "config.json", "r", encoding="utf-8") as fh:
            cfg = json.load(fh)
        backend_cls = getattr(_backends, cfg.get("backend_type", "ExactIndex"), ExactIndex)
        if backend_cls in (HNSWIndex, FAISSIndex):
            backend_cls = ExactIndex  # graph files are not readable here; the exact index serves the same rows
        inst = cls(dim=cfg["dim"], space=cfg["space"], backend="exact", use_ann=cfg.get("use_ann", True),
                   ef_query=cfg.get("ef_query", 200), rerank_eta=cfg.get("rerank_eta", 0.25),
                   entropy_pref=cfg.get("entropy_pref", 0.0))
        exact_kwargs = {k: v for k, v in kwargs.items() if k in ("device", "batch_shadow", "shadow_single_query", "int8_shadow", "binary_shadow")}
        inst._backend = backend_cls.load(root / "ann_index", **exact_kwargs)
        inst._built = False  # device copy is rebuilt on first use
        meta_path = root / "meta.json"
        if meta_path.exists():
            with open(meta_path, "r", encoding="utf-8") as fh:
                inst._meta = json.load(fh)
        return inst


__all__ = ["DewiIndex", "BaseIndex", "ExactIndex", "HNSWIndex", "FAISSIndex", "IndexBackend", "_HAS_FAISS",
           "_HAS_HNSW", "Payload"]

"""Hybrid search service: per-node indexing, BM25 + vector + RRF + MMR.

Parity: reference pkg/search/search.go Service (:236): per-node indexing
(:651), BuildIndexes (:767), hybrid Search (:851), RRF fusion (:1432),
MMR diversification (:1544), type filters. Stays in sync with storage via
event callbacks (reference pkg/nornicdb/db.go:994-1035 wiring).
"""

from __future__ import annotations

import threading
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..storage.types import Engine, EventType, Node
from .bm25 import FulltextIndex
from .bm25_device import DeviceFulltextIndex
from .embedding_index import EmbeddingIndex
from .fusion import mmr_diversify, rrf_fuse
from .hnsw import HNSWIndex
from .ivf import IVFIndex
from .kmeans import ClusterIndex, optimal_k
from .pipeline import KMEANS_MIN, VectorSearchPipeline

TEXT_PROPS = ("title", "name", "content", "text", "description", "summary", "body")


def node_text(node: Node) -> str:
    parts = []
    for p in TEXT_PROPS:
        v = node.properties.get(p)
        if isinstance(v, str):
            parts.append(v)
    return " ".join(parts)


@dataclass
class SearchResult:
    id: str
    score: float
    node: Optional[Node] = None
    source: str = "hybrid"


class SearchService:
    def __init__(self, engine: Engine, dims: int = 1024,
                 device: Optional[str] = None, use_hnsw: bool = True,
                 embedder=None, quant: Optional[str] = None,
                 ivf: bool = False, fulltext_gpu: bool = False):
        self.engine = engine
        self.dims = dims
        self.embedder = embedder
        self._lock = threading.RLock()
        self.fulltext = FulltextIndex()
        # NORNICDB_SEARCH_QUANT=int8|fp8 stores the GPU corpus at
        # 1 B/element (half the HBM traffic, 2x capacity). int8 keeps
        # per-row scales (~7 bits, recall@10 >= 0.95 worst-case); fp8
        # e4m3 is scale-free but coarser (~0.91 worst-case)
        import os as _os
        quant = quant or _os.environ.get("NORNICDB_SEARCH_QUANT") or None
        self.emb = EmbeddingIndex(dims, device=device, quant=quant)
        self.hnsw = HNSWIndex(dims) if use_hnsw else None
        self.clusters = ClusterIndex()
        # opt-in device-resident IVF search (ivf=True or
        # NORNICDB_SEARCH_IVF=1): recluster() also freezes the clusters as
        # inverted lists on the device, and the pipeline routes large
        # corpora (or any query that passes nprobe) to them
        ivf = ivf or _os.environ.get("NORNICDB_SEARCH_IVF") == "1"
        self.ivf = IVFIndex(self.emb) if ivf else None
        # opt-in device-resident BM25 (fulltext_gpu=True or
        # NORNICDB_SEARCH_FULLTEXT_GPU=1): build_indexes() freezes the
        # postings on the device, text queries are scored there, and
        # recluster() rebuilds them once enough documents have changed
        fulltext_gpu = fulltext_gpu or \
            _os.environ.get("NORNICDB_SEARCH_FULLTEXT_GPU") == "1"
        self.fulltext_dev = (DeviceFulltextIndex(self.fulltext, device=device)
                             if fulltext_gpu else None)
        self.pipeline = VectorSearchPipeline(self.emb, self.hnsw,
                                             self.clusters, ivf=self.ivf)
        # label -> ids of nodes with an embedding; the vector path turns a
        # label predicate into the kNN allow-mask instead of over-fetching
        self._label_ids: Dict[str, set] = {}
        self._node_labels: Dict[str, Tuple[str, ...]] = {}
        engine.register_callback(self._on_event)

    # ---- storage sync ----
    def _on_event(self, ev: str, obj: Any):
        if ev in (EventType.NODE_CREATED, EventType.NODE_UPDATED):
            self.index_node(obj)
        elif ev == EventType.NODE_DELETED:
            self.remove_node(obj.id)

    def index_node(self, node: Node):
        with self._lock:
            text = node_text(node)
            if text:
                self.fulltext.index(node.id, text)
            has_vec = (node.embedding is not None
                       and len(node.embedding) == self.dims)
            if has_vec or node.id in self._node_labels:
                # also on an update that carries no embedding: the vector
                # indexed earlier stays searchable under the new labels
                self._set_labels(node.id, node.labels)
            if has_vec:
                self.emb.add(node.id, node.embedding)
                if self.hnsw is not None and len(self.emb) <= KMEANS_MIN:
                    self.hnsw.add(node.id, node.embedding)
                self.clusters.add(node.id, node.embedding)

    def remove_node(self, node_id: str):
        with self._lock:
            self.fulltext.remove(node_id)
            self._set_labels(node_id, ())
            self._node_labels.pop(node_id, None)
            self.emb.remove(node_id)
            if self.hnsw is not None:
                self.hnsw.remove(node_id)
            self.clusters.remove(node_id)

    def _set_labels(self, node_id: str, labels: Sequence[str]):
        """Move node_id into exactly the sets of `labels` (a NODE_UPDATED
        that changes labels leaves the old sets)."""
        new = tuple(labels or ())
        old = self._node_labels.get(node_id, ())
        for lb in old:
            if lb not in new:
                ids = self._label_ids.get(lb)
                if ids is not None:
                    ids.discard(node_id)
                    if not ids:
                        del self._label_ids[lb]
        for lb in new:
            self._label_ids.setdefault(lb, set()).add(node_id)
        self._node_labels[node_id] = new

    def _allow_ids(self, labels: Sequence[str]) -> Optional[set]:
        """Union of the label sets, or None without a label predicate."""
        if not labels:
            return None
        with self._lock:
            out: set = set()
            for lb in labels:
                out |= self._label_ids.get(lb, set())
            return out

    def build_indexes(self):
        """Full scan (reference BuildIndexes)."""
        for node in self.engine.all_nodes():
            self.index_node(node)
        if self.fulltext_dev is not None:
            self.fulltext_dev.build()

    def recluster(self, k: int = None):
        if self.fulltext_dev is not None and self.fulltext_dev.needs_rebuild():
            self.fulltext_dev.build()
        ids = self.emb.ids()
        if not ids:
            return
        with self._lock:
            mat = self.emb.matrix().float()
            slot_ids = [i for i in self.emb._ids if i in self.emb._id2slot]
            self.clusters.cluster(slot_ids, mat[: len(self.emb._ids)],
                                  k=k or optimal_k(len(slot_ids)))
            if self.ivf is not None:
                self.ivf.build(n_lists=k)

    # ---- queries ----
    def vector_search(self, query_vec, k: int = 10,
                      labels: Sequence[str] = None,
                      nprobe: Optional[int] = None) -> List[SearchResult]:
        """nprobe: IVF lists to probe; only read when IVF is enabled."""
        hits = self.pipeline.search(np.asarray(query_vec, np.float32), k,
                                    allow_ids=self._allow_ids(labels),
                                    nprobe=nprobe)
        return self._materialize(hits, k, labels, source="vector")

    def _fulltext_search(self, query: str, k: int):
        """BM25 hits from the device index when it is enabled (it
        delegates to the host index until it is built)."""
        ft = self.fulltext_dev if self.fulltext_dev is not None \
            else self.fulltext
        return ft.search(query, k)

    def text_search(self, query: str, k: int = 10,
                    labels: Sequence[str] = None) -> List[SearchResult]:
        hits = self._fulltext_search(query, k * 3 if labels else k)
        return self._materialize(hits, k, labels, source="fulltext")

    def search(self, query: str = None, query_vec=None, k: int = 10,
               labels: Sequence[str] = None, mmr: bool = False,
               mmr_lambda: float = 0.7,
               nprobe: Optional[int] = None) -> List[SearchResult]:
        """Hybrid search: BM25 + vector fused with RRF; optional MMR.
        nprobe: IVF lists to probe; only read when IVF is enabled."""
        if query_vec is None and query and self.embedder is not None:
            query_vec = self.embedder.embed_query(query)
        rankings = []
        if query:
            rankings.append(self._fulltext_search(query, max(k * 4, 40)))
        if query_vec is not None and len(self.emb) > 0:
            rankings.append(self.pipeline.search(
                np.asarray(query_vec, np.float32), max(k * 4, 40),
                allow_ids=self._allow_ids(labels), nprobe=nprobe))
        if not rankings:
            return []
        if len(rankings) == 1:
            fused = rankings[0]
        else:
            fused = rrf_fuse(rankings)
        if mmr and query_vec is not None:
            vecs = {}
            for id_, _ in fused[: max(k * 4, 40)]:
                v = self.emb.get(id_)
                if v is not None:
                    vecs[id_] = v
            fused = mmr_diversify(fused[: max(k * 4, 40)], vecs, k * 3,
                                  lambda_=mmr_lambda)
        return self._materialize(fused, k, labels, source="hybrid")

    def _materialize(self, hits: List[Tuple[str, float]], k: int,
                     labels: Sequence[str], source: str) -> List[SearchResult]:
        out = []
        for id_, score in hits:
            try:
                node = self.engine.get_node(id_)
            except Exception:
                continue
            if labels and not any(lb in node.labels for lb in labels):
                continue
            out.append(SearchResult(id_, float(score), node, source))
            if len(out) >= k:
                break
        return out

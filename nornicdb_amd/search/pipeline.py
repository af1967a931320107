"""Vector search pipeline: candidate generation x exact scoring.

Parity: reference pkg/search/vector_pipeline.go — brute force below 5K
vectors (:22-24), HNSW in the mid range, k-means cluster routing above
100K (kmeans_candidate_gen.go), candidate set max(20k, 200) capped at
5000 (:26-31), exact re-scoring on GPU (:236 GPUExactScorer). An opt-in
IVFIndex (search/ivf.py) replaces the host-side cluster routing with
inverted lists scanned on the device.
"""

from __future__ import annotations

from typing import Iterable, List, Optional, Tuple

from .embedding_index import EmbeddingIndex
from .hnsw import HNSWIndex
from .ivf import IVFIndex
from .kmeans import ClusterIndex

BRUTE_MAX = 5_000
KMEANS_MIN = 100_000


def candidate_count(k: int) -> int:
    return min(max(20 * k, 200), 5000)


class VectorSearchPipeline:
    def __init__(self, emb: EmbeddingIndex, hnsw: Optional[HNSWIndex] = None,
                 clusters: Optional[ClusterIndex] = None,
                 ivf: Optional[IVFIndex] = None):
        self.emb = emb
        self.hnsw = hnsw
        self.clusters = clusters
        self.ivf = ivf

    def search(self, query, k: int,
               allow_ids: Optional[Iterable[str]] = None,
               nprobe: Optional[int] = None
               ) -> List[Tuple[str, float]]:
        """allow_ids restricts hits to those ids: the brute-force branches
        filter inside the kNN kernel; the HNSW and cluster branches
        intersect their candidates with it and fall back to the filtered
        brute-force search when fewer than k survive.

        With a built IVFIndex, corpora above KMEANS_MIN (or any call that
        passes nprobe) are served by the device-resident IVF search, which
        applies allow_ids inside its kernel. Without one, nprobe is
        ignored."""
        n = len(self.emb)
        if n == 0:
            return []
        if allow_ids is not None and not isinstance(allow_ids, (set, frozenset)):
            allow_ids = set(allow_ids)
        if self.ivf is not None and self.ivf.built and (
                n > KMEANS_MIN or nprobe is not None):
            return self.ivf.search(query, k, nprobe=nprobe,
                                   allow_ids=allow_ids)
        # brute force: small corpora, or GPU path (fused kernel IS the fast path)
        if n <= BRUTE_MAX or (self.emb.device.type == "cuda"
                              and (self.clusters is None or self.clusters.k == 0)):
            return self.emb.search(query, k, allow_ids=allow_ids)
        if n > KMEANS_MIN and self.clusters is not None and self.clusters.k > 0:
            cands = self.clusters.candidates(query)
            if len(cands) > candidate_count(k):
                # HNSW narrows within the routed set if available, else truncate
                cands = cands[: candidate_count(k) * 4]
            if allow_ids is not None:
                cands = [i for i in cands if i in allow_ids]
                if len(cands) < k:
                    return self.emb.search(query, k, allow_ids=allow_ids)
            scored = self.emb.score_subset(query, cands)
            return scored[:k]
        if self.hnsw is not None and len(self.hnsw) > 0:
            cands = [i for i, _ in self.hnsw.search(query, candidate_count(k))]
            if allow_ids is not None:
                cands = [i for i in cands if i in allow_ids]
                if len(cands) < k:
                    return self.emb.search(query, k, allow_ids=allow_ids)
            scored = self.emb.score_subset(query, cands)
            return scored[:k]
        return self.emb.search(query, k, allow_ids=allow_ids)

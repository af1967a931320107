"""Device-resident IVF index over an EmbeddingIndex.

`build()` runs k-means over the live slots and freezes the clusters as
inverted lists of slot numbers on the embedding index's device
(ops.ivf.IVFLists). A search routes the query to its `nprobe` nearest
centroids and scores only those lists plus the tail, the slots appended
since the build, with a fused scan kernel on the GPU: `ivf_scan` for a
bf16 corpus, `ivf_scan_i8` / `ivf_scan_fp8` for the quantised modes
(ops.ivf.ivf_route_kind). The corpus is not copied or reordered, and the index's own live mask (ANDed with any
`allow_ids`) is the kernel's allow mask, so removed ids are never returned
and never widen k.

Parity: reference pkg/search/kmeans_candidate_gen.go
ClusterIndex.SearchWithClusters(query, limit, numClusters); the reference
keeps cluster members as host-side id lists.
"""

from __future__ import annotations

from typing import Iterable, List, Optional, Tuple

import numpy as np
import torch

from ..ops.ivf import IVFLists, ivf_build_lists, ivf_route, ivf_search
from .embedding_index import EmbeddingIndex
from .kmeans import kmeans, optimal_k

REBUILD_RATIO = 0.2   # same drift ratio as ClusterIndex.needs_recluster


class IVFIndex:
    def __init__(self, emb: EmbeddingIndex, nprobe: int = 8):
        if getattr(emb, "metric", "cosine") != "cosine":
            # the scan kernels and the centroid routing score inner products
            # of normalised vectors only
            raise ValueError(
                f"IVFIndex needs a cosine EmbeddingIndex, got metric "
                f"{emb.metric!r}")
        self.emb = emb
        self._lock = emb._lock         # one lock for vectors and lists
        self._nprobe = nprobe
        self._lists: Optional[IVFLists] = None
        self._stale: set = set()
        emb._overwrite_hooks.append(self._on_overwrite)

    # ---- state ----
    @property
    def built(self) -> bool:
        return self._lists is not None

    @property
    def n_lists(self) -> int:
        return 0 if self._lists is None else self._lists.n_lists

    @property
    def nprobe(self) -> int:
        return self._nprobe

    @property
    def n_built(self) -> int:
        return 0 if self._lists is None else self._lists.n_built

    @property
    def tail(self) -> int:
        """Slots appended since build(); every search scans them."""
        return 0 if self._lists is None else self.emb._n - self._lists.n_built

    @property
    def stale(self) -> int:
        """Slots below n_built overwritten since build(): still scored
        exactly, but listed under the cluster of their old vector."""
        return len(self._stale)

    def needs_rebuild(self) -> bool:
        with self._lock:
            if self._lists is None:
                return False
            return (self.tail + self.stale) > REBUILD_RATIO * self.n_built

    def _on_overwrite(self, slot: int):
        if self._lists is not None and slot < self._lists.n_built:
            self._stale.add(slot)

    # ---- build ----
    def build(self, n_lists: Optional[int] = None, iters: int = 25,
              seed: int = 0) -> None:
        """Cluster the live slots and freeze the inverted lists. Dead slots
        go in no list."""
        emb = self.emb
        with self._lock:
            n = emb._n
            live = np.flatnonzero(emb._live[:n])
            if live.size == 0:
                self._lists = None
                self._stale = set()
                return
            slots = torch.from_numpy(live).to(emb.device)
            x = emb.matrix()
            x = x if live.size == n else x[slots]
            c, assign = kmeans(x, n_lists or optimal_k(live.size),
                               iters=iters, seed=seed)
            full = torch.full((n,), -1, dtype=torch.int64, device=emb.device)
            full[slots] = assign.to(torch.int64)
            self._lists = ivf_build_lists(full, c.shape[0], n, c)
            self._stale = set()

    # ---- search ----
    def _search(self, q: torch.Tensor, k: int, nprobe: int, allow_ids):
        emb = self.emb
        n = emb._n
        lists = self._lists
        probes = ivf_route(lists, q, nprobe)
        # int8 takes the float query (quantised behind ivf_search) and the
        # row scales
        int8 = emb.quant == "int8"
        return ivf_search(emb._buf[:n], q if int8 else q.to(emb.dtype),
                          min(k, n), lists, probes, lists.n_built,
                          allow=emb._allow_mask(allow_ids),
                          scales=emb._scales[:n] if int8 else None)

    def _delegates(self, nprobe: int) -> bool:
        return self._lists is None or nprobe >= self._lists.n_lists

    def search(self, query, k: int, nprobe: Optional[int] = None,
               allow_ids: Optional[Iterable[str]] = None
               ) -> List[Tuple[str, float]]:
        """Top-k over the nprobe nearest lists and the tail. Same result
        type as EmbeddingIndex.search; not built, or nprobe >= n_lists,
        is the brute-force search."""
        with self._lock:
            nprobe = nprobe or self._nprobe
            if self._delegates(nprobe):
                return self.emb.search(query, k, allow_ids=allow_ids)
            if self.emb._n == 0:
                return []
            q = torch.as_tensor(np.asarray(query, dtype=np.float32),
                                device=self.emb.device).reshape(1, -1)
            q = self.emb._normalize(q)
            s, i = self._search(q, k, nprobe, allow_ids)
            return self.emb._hits(s[0], i[0], k)

    def search_batch(self, queries, k: int, nprobe: Optional[int] = None,
                     allow_ids: Optional[Iterable[str]] = None
                     ) -> List[List[Tuple[str, float]]]:
        with self._lock:
            nprobe = nprobe or self._nprobe
            if self._delegates(nprobe):
                return self.emb.search_batch(queries, k, allow_ids=allow_ids)
            if self.emb._n == 0:
                return [[] for _ in range(len(queries))]
            q = torch.as_tensor(np.asarray(queries, dtype=np.float32),
                                device=self.emb.device)
            q = self.emb._normalize(q)
            s, i = self._search(q, k, nprobe, allow_ids)
            return [self.emb._hits(s[r], i[r], k) for r in range(q.shape[0])]

"""GPU-resident embedding matrix with top-k scoring.

Replaces reference pkg/gpu/gpu.go EmbeddingIndex (:1224: dirty-tracking
auto-sync, ScoreSubset :1554) with a single CDNA4 path: vectors live in a
bf16 torch tensor on the MI355X (fp32 numpy on CPU test runs), scored by
the fused HIP kNN kernels (ops.knn_search). No multi-backend probing.

Metric (reference pkg/qdrantgrpc/vector_index_cache.go, pkg/math/vector/
similarity.go): `cosine` L2-normalises rows and queries and scores inner
products; `dot` stores and scores vectors as given; `euclidean` stores
vectors as given beside a per-row bias -|x|^2/2, so that the kernels' inner
product plus bias ranks by distance (argmax q.x - |x|^2/2 = argmin |q-x|),
then re-scores the k hits exactly and returns 1 / (1 + distance).
"""

from __future__ import annotations

import threading
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .vectorspace import COSINE, EUCLIDEAN, normalize_metric


class EmbeddingIndex:
    def __init__(self, dims: int, device: Optional[str] = None,
                 capacity: int = 1024, quant: Optional[str] = None,
                 metric: str = COSINE):
        self.dims = dims
        self.metric = normalize_metric(metric)
        if quant is not None and self.metric != COSINE:
            raise ValueError(
                f"metric {self.metric!r} needs an unquantised index: "
                f"quant={quant!r} corpora score cosine only")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        # quant="fp8": store vectors as OCP e4m3fn — half the HBM traffic
        # and 2x capacity (200M+ 1024-d per 288 GB GPU), scored by the
        # fp8 MFMA kernel (csrc/knn_q8.hip); ~1% recall@10 cost on
        # normalized vectors. No reference analogue (pkg/gpu is fp32).
        self.quant = quant
        if quant == "fp8":
            self.dtype = torch.float8_e4m3fn
        elif quant == "int8":
            # symmetric per-row int8 (recommended): ~7 effective bits,
            # scored by the i8 MFMA at 2x the bf16 rate
            self.dtype = torch.int8
        elif quant is not None:
            raise ValueError(f"unknown quant mode {quant!r}")
        else:
            self.dtype = (torch.bfloat16 if self.device.type == "cuda"
                          else torch.float32)
        self._lock = threading.RLock()
        self._buf = torch.zeros(capacity, dims, device=self.device, dtype=self.dtype)
        self._scales = (torch.zeros(capacity, device=self.device)
                        if quant == "int8" else None)
        # euclidean: -|row|^2 / 2 of the stored (rounded) row, fp32, kept in
        # step with _buf: written wherever a row is written
        self._bias = (torch.zeros(capacity, device=self.device)
                      if self.metric == EUCLIDEAN else None)
        self._n = 0
        self._ids: List[str] = []
        self._id2slot: Dict[str, int] = {}
        self._dead: set = set()
        # host-side bit per slot: set while the slot holds a live vector.
        # Searches pass it (ANDed with any allow_ids filter) to the kNN
        # kernels as the allow-mask, so tombstones never widen k. The
        # device copy is re-packed lazily on the next search after a change.
        self._live = np.zeros(capacity, dtype=bool)
        self._live_dirty = True
        self._live_words: Optional[torch.Tensor] = None
        # called with the slot when add()/add_batch() overwrite a stored
        # vector in place (IVFIndex counts such slots as stale)
        self._overwrite_hooks: List = []

    def __len__(self):
        return self._n - len(self._dead)

    def _grow(self, need: int):
        cap = self._buf.shape[0]
        if need <= cap:
            return
        new_cap = max(need, cap * 2)
        nb = torch.zeros(new_cap, self.dims, device=self.device, dtype=self.dtype)
        nb[:self._n] = self._buf[:self._n]
        self._buf = nb
        if self._scales is not None:
            ns = torch.zeros(new_cap, device=self.device)
            ns[:self._n] = self._scales[:self._n]
            self._scales = ns
        if self._bias is not None:
            nbias = torch.zeros(new_cap, device=self.device)
            nbias[:self._n] = self._bias[:self._n]
            self._bias = nbias
        nl = np.zeros(new_cap, dtype=bool)
        nl[:self._n] = self._live[:self._n]
        self._live = nl

    @staticmethod
    def _normalize(t: torch.Tensor) -> torch.Tensor:
        t = t.float()
        return t / torch.linalg.vector_norm(t, dim=-1, keepdim=True).clamp_min(1e-12)

    def _prep(self, t: torch.Tensor) -> torch.Tensor:
        """Rows or queries as the metric scores them: L2-normalised for
        cosine, as given for dot and euclidean (fp32 either way)."""
        return self._normalize(t) if self.metric == COSINE else t.float()

    def _store_rows(self, m: torch.Tensor):
        """prepared fp32 rows -> (rows in storage dtype, scales|None)"""
        if self.quant == "int8":
            from ..ops.knn import quantize_int8
            return quantize_int8(m)
        return m.to(self.dtype), None

    def _write_row(self, slot: int, row: torch.Tensor, scale) -> None:
        """The one place a stored row changes: row, scale and bias together."""
        self._buf[slot] = row
        if scale is not None:
            self._scales[slot] = scale
        if self._bias is not None:
            self._bias[slot] = -0.5 * row.float().square().sum()

    def add(self, id_: str, vec) -> None:
        with self._lock:
            v = torch.as_tensor(np.asarray(vec, dtype=np.float32),
                                device=self.device)
            v, sc = self._store_rows(self._prep(v.reshape(1, -1)))
            slot = self._id2slot.get(id_)
            if slot is not None:
                self._write_row(slot, v[0], None if sc is None else sc[0])
                self._dead.discard(slot)
                self._set_live(slot, True)
                for hook in self._overwrite_hooks:
                    hook(slot)
                return
            self._grow(self._n + 1)
            self._write_row(self._n, v[0], None if sc is None else sc[0])
            self._ids.append(id_)
            self._id2slot[id_] = self._n
            self._set_live(self._n, True)
            self._n += 1

    def add_batch(self, ids: Sequence[str], mat) -> None:
        with self._lock:
            m = torch.as_tensor(np.asarray(mat, dtype=np.float32), device=self.device)
            m, sc = self._store_rows(self._prep(m))
            self._grow(self._n + len(ids))
            for i, id_ in enumerate(ids):
                slot = self._id2slot.get(id_)
                if slot is not None:
                    self._write_row(slot, m[i], None if sc is None else sc[i])
                    self._dead.discard(slot)
                    self._set_live(slot, True)
                    for hook in self._overwrite_hooks:
                        hook(slot)
                else:
                    self._write_row(self._n, m[i],
                                    None if sc is None else sc[i])
                    self._ids.append(id_)
                    self._id2slot[id_] = self._n
                    self._set_live(self._n, True)
                    self._n += 1

    def remove(self, id_: str) -> bool:
        with self._lock:
            slot = self._id2slot.pop(id_, None)
            if slot is None:
                return False
            self._dead.add(slot)
            self._set_live(slot, False)
            return True

    def _set_live(self, slot: int, on: bool):
        self._live[slot] = on
        self._live_dirty = True

    def _allow_mask(self, allow_ids: Optional[Iterable[str]]):
        """Packed allow-mask for the next kNN call, or None when every slot
        may be returned (no tombstones, no filter)."""
        if allow_ids is None:
            if not self._dead:
                return None
            if self._live_dirty:
                self._live_words = self._upload_mask(self._live[:self._n])
                self._live_dirty = False
            return self._live_words
        # live & allow_ids: _id2slot only knows live ids, unknown ids drop out
        ok = np.zeros(self._n, dtype=bool)
        slots = [self._id2slot[i] for i in allow_ids if i in self._id2slot]
        ok[slots] = True
        return self._upload_mask(ok)

    def _upload_mask(self, ok: np.ndarray) -> torch.Tensor:
        """Host bool per slot -> packed words on the device (packed on the
        host, so 1 bit per slot crosses the bus)."""
        from ..ops.knn import pack_allow_mask

        return pack_allow_mask(torch.from_numpy(ok)).to(self.device)

    def _knn(self, q: torch.Tensor, k: int, allow_ids):
        from ..ops import knn_search

        kk = min(k, self._n)
        mask = self._allow_mask(allow_ids)     # None: the unfiltered route
        db = self._buf[:self._n]
        if self.quant == "int8":
            from ..ops.knn import knn_search_int8
            return knn_search_int8(db, self._scales[:self._n], q, kk,
                                   allow=mask)
        if self._bias is None:
            return knn_search(db, q.to(self.dtype), kk, allow=mask)
        s, i = knn_search(db, q.to(self.dtype), kk, allow=mask,
                          row_bias=self._bias[:self._n])
        return self._rescore_euclidean(q, i)

    def _rescore_euclidean(self, q: torch.Tensor, i: torch.Tensor):
        """Exact scores for the slots a biased search returned: fp32
        |q - row| against the stored rows, re-sorted ascending, returned as
        1 / (1 + distance) (descending). The kernel's q.x - |x|^2/2 only
        ranks: turning it back into a distance, |q|^2 - 2s, cancels for near
        duplicates. Unfilled slots (index -1) stay last with score -inf."""
        rows = self._buf[i.clamp_min(0)].float()           # [Q, k, D]
        dist = torch.linalg.vector_norm(q.float()[:, None, :] - rows, dim=-1)
        dist = dist.masked_fill(i < 0, float("inf"))
        dist, order = torch.sort(dist, dim=-1, stable=True)
        i = torch.gather(i, -1, order)
        score = (1.0 / (1.0 + dist)).masked_fill(i < 0, float("-inf"))
        return score, i

    def _hits(self, scores, slots, k: int) -> List[Tuple[str, float]]:
        """One query's (scores, slots) as [(id, score)]: the first k that
        are neither unfilled (slot < 0) nor dead."""
        out = []
        for score, slot in zip(scores.tolist(), slots.tolist()):
            if slot < 0 or slot in self._dead:
                continue
            out.append((self._ids[slot], float(score)))
            if len(out) >= k:
                break
        return out

    def search(self, query, k: int,
               allow_ids: Optional[Iterable[str]] = None
               ) -> List[Tuple[str, float]]:
        """Brute-force top-k over all vectors (fused HIP kernel on GPU).

        allow_ids restricts the hits to those ids (unknown ids are
        ignored); the filter runs inside the kNN kernel."""
        with self._lock:
            if self._n == 0:
                return []
            q = torch.as_tensor(np.asarray(query, dtype=np.float32),
                                device=self.device).reshape(1, -1)
            q = self._prep(q)
            s, i = self._knn(q, k, allow_ids)
            return self._hits(s[0], i[0], k)

    def search_batch(self, queries, k: int,
                     allow_ids: Optional[Iterable[str]] = None
                     ) -> List[List[Tuple[str, float]]]:
        with self._lock:
            if self._n == 0:
                return [[] for _ in range(len(queries))]
            q = torch.as_tensor(np.asarray(queries, dtype=np.float32),
                                device=self.device)
            q = self._prep(q)
            s, i = self._knn(q, k, allow_ids)
            return [self._hits(s[r], i[r], k) for r in range(q.shape[0])]

    def score_subset(self, query, ids: Sequence[str]) -> List[Tuple[str, float]]:
        """Exact re-scoring of a candidate subset (reference ScoreSubset)."""
        with self._lock:
            slots = [self._id2slot[i] for i in ids if i in self._id2slot]
            if not slots:
                return []
            q = torch.as_tensor(np.asarray(query, dtype=np.float32),
                                device=self.device).reshape(-1)
            q = self._prep(q.reshape(1, -1))[0]
            sl = torch.as_tensor(slots, device=self.device)
            sub = self._buf[sl].float()
            if self._scales is not None:
                sub = sub * self._scales[sl, None]
            if self.metric == EUCLIDEAN:
                dist = torch.linalg.vector_norm(sub - q.float(), dim=-1)
                scores = (1.0 / (1.0 + dist)).tolist()
            else:
                scores = (sub @ q.float()).tolist()
            kept = [i for i in ids if i in self._id2slot]
            return sorted(zip(kept, scores), key=lambda kv: -kv[1])

    def get(self, id_: str) -> Optional[np.ndarray]:
        with self._lock:
            slot = self._id2slot.get(id_)
            if slot is None:
                return None
            v = self._buf[slot].float()
            if self._scales is not None:
                v = v * self._scales[slot]
            return v.cpu().numpy()

    def ids(self) -> List[str]:
        with self._lock:
            return [i for i in self._ids if i in self._id2slot]

    def matrix(self) -> torch.Tensor:
        with self._lock:
            m = self._buf[:self._n]
            if self._scales is not None:
                # int8 storage: return dequantized values — callers
                # (recluster/k-means) expect real vector magnitudes
                return m.float() * self._scales[:self._n, None]
            return m

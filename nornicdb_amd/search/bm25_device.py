"""Device-resident BM25 index over a FulltextIndex.

`build()` gives every current document a slot, freezes the vocabulary
(term -> id) and uploads the postings as a CSR of slot numbers
(ops.bm25.BM25Postings); a search scores them with the fused `bm25_scan`
kernel on the GPU. The host FulltextIndex stays the source of truth and
follows the life-cycle of IVFIndex: a document changed or removed after the
build has its frozen slot's live bit cleared (*stale*), a document that
exists now and was indexed after the build is in the *tail*, a host-side
set scored with the host formula on every search, and `build()` folds both
back in once `needs_rebuild()`.

Every search takes n_docs, avg_len and each term's df from the host index as
it is NOW, so frozen and tail documents are scored with identical
statistics, the ones `FulltextIndex.search` uses.

Parity: reference pkg/search/fulltext_index.go keeps host maps only.
"""

from __future__ import annotations

from collections import Counter
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops.bm25 import BM25Postings, bm25_build_postings, bm25_search
from ..ops.knn import pack_allow_mask
from .bm25 import FulltextIndex, tokenize

REBUILD_RATIO = 0.2   # same drift ratio as IVFIndex.needs_rebuild


class DeviceFulltextIndex:
    def __init__(self, ft: FulltextIndex, device: Optional[str] = None):
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.ft = ft
        self.device = torch.device(device)
        self._lock = ft._lock          # one lock for the host and device halves
        self._post: Optional[BM25Postings] = None
        self._vocab: dict = {}         # term -> frozen term id
        self._ids: List[str] = []      # slot -> doc id
        self._slot: dict = {}          # doc id -> slot
        self._live = np.zeros(0, dtype=bool)
        self._n_stale = 0
        self._tail: set = set()
        self._live_words: Optional[torch.Tensor] = None   # packed, on device
        ft._change_hooks.append(self._on_change)

    # ---- state ----
    @property
    def built(self) -> bool:
        return self._post is not None

    @property
    def n_built(self) -> int:
        return len(self._ids)

    @property
    def tail(self) -> int:
        """Documents indexed since build(); scored on the host."""
        return len(self._tail)

    @property
    def stale(self) -> int:
        """Frozen slots whose document changed or left since build()."""
        return self._n_stale

    def needs_rebuild(self) -> bool:
        with self._lock:
            if self._post is None:
                return False
            return (self.tail + self.stale) > REBUILD_RATIO * self.n_built

    def _on_change(self, doc_id: str):
        if self._post is None:
            return
        slot = self._slot.get(doc_id)
        if slot is not None and self._live[slot]:
            self._live[slot] = False
            self._n_stale += 1
            self._live_words = None
        if doc_id in self.ft._doc_len:
            self._tail.add(doc_id)
        else:
            self._tail.discard(doc_id)

    # ---- build ----
    def build(self) -> None:
        """Slot every current document (insertion order), freeze the
        vocabulary and upload the postings."""
        ft = self.ft
        with self._lock:
            self._tail = set()
            self._n_stale = 0
            self._live_words = None
            self._ids = list(ft._doc_len)
            self._slot = {d: s for s, d in enumerate(self._ids)}
            self._live = np.ones(len(self._ids), dtype=bool)
            if not self._ids:
                self._post, self._vocab = None, {}
                return
            slot = self._slot
            self._vocab = {t: i for i, t in enumerate(ft._postings)}
            term_docs = [{slot[d]: tf for d, tf in posting.items()}
                         for posting in ft._postings.values()]
            self._post = bm25_build_postings(
                term_docs, [ft._doc_len[d] for d in self._ids], self.device)

    # ---- search ----
    def _allow_mask(self, allow_ids) -> Optional[torch.Tensor]:
        """Packed live AND allowed slots on the device; None when every
        slot may be returned."""
        if allow_ids is None:
            if self._n_stale == 0:
                return None
            if self._live_words is None:
                self._live_words = pack_allow_mask(
                    torch.from_numpy(self._live)).to(self.device)
            return self._live_words
        ok = np.zeros(len(self._ids), dtype=bool)
        slots = [self._slot[d] for d in allow_ids if d in self._slot]
        ok[slots] = True
        ok &= self._live
        return pack_allow_mask(torch.from_numpy(ok)).to(self.device)

    def _query_columns(self, toks: Sequence[str]):
        """(frozen term ids, weights) of the distinct query terms the host
        index holds now, w = count * idf * (k1 + 1); a term the frozen
        vocabulary lacks gets id -1 and is scored in the tail alone."""
        ft = self.ft
        n_docs = len(ft._doc_len)
        ids, ws = [], []
        for term, count in Counter(toks).items():
            posting = ft._postings.get(term)
            if not posting:
                continue
            ids.append(self._vocab.get(term, -1))
            ws.append(count * ft.idf(n_docs, len(posting)) * (ft.k1 + 1))
        return ids, ws

    def search_batch(self, queries: Sequence[str], k: int = 10,
                     allow_ids: Optional[Iterable[str]] = None
                     ) -> List[List[Tuple[str, float]]]:
        ft = self.ft
        with self._lock:
            if self._post is None or not ft._doc_len:
                hits = [ft.search(q, k) if allow_ids is None else
                        self._host_search(q, k, allow_ids) for q in queries]
                return hits
            if not queries:
                return []
            allow_set = None if allow_ids is None else set(allow_ids)
            toks = [tokenize(q) for q in queries]
            cols = [self._query_columns(t) for t in toks]
            width = max(1, max(len(ids) for ids, _ in cols))
            q_terms = np.full((len(queries), width), -1, dtype=np.int32)
            q_w = np.zeros((len(queries), width), dtype=np.float32)
            for r, (ids, ws) in enumerate(cols):
                q_terms[r, :len(ids)] = ids
                q_w[r, :len(ws)] = ws
            avg_len = ft._total_len / len(ft._doc_len)
            c0 = ft.k1 * (1 - ft.b)
            c1 = ft.k1 * ft.b / avg_len
            s, i = bm25_search(
                self._post, torch.from_numpy(q_terms).to(self.device),
                torch.from_numpy(q_w).to(self.device), c0, c1,
                min(k, len(self._ids)), allow=self._allow_mask(allow_set))
            s, i = s.tolist(), i.tolist()
            tail = self._tail if allow_set is None else \
                self._tail & allow_set
            out = []
            for r in range(len(queries)):
                hits = [(self._ids[slot], sc) for sc, slot in zip(s[r], i[r])
                        if slot >= 0]
                if tail:
                    hits += ft.score_terms(toks[r], docs=tail).items()
                    hits.sort(key=lambda kv: -kv[1])
                out.append(hits[:k])
            return out

    def search(self, query: str, k: int = 10,
               allow_ids: Optional[Iterable[str]] = None
               ) -> List[Tuple[str, float]]:
        """Top-k (id, score) of the frozen, live documents and the tail;
        the same result type as FulltextIndex.search. Not built, or an
        empty index, is the host search."""
        return self.search_batch([query], k, allow_ids=allow_ids)[0]

    def _host_search(self, query: str, k: int, allow_ids):
        allow_set = set(allow_ids)
        scores = self.ft.score_terms(tokenize(query), docs=allow_set & set(
            self.ft._doc_len))
        return sorted(scores.items(), key=lambda kv: -kv[1])[:k]

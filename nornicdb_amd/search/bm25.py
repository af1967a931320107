"""BM25 full-text index.

Parity: reference pkg/search/fulltext_index.go (:20,:125,:205; tokenizer +
stopwords :249-287). k1=1.2, b=0.75.
"""

from __future__ import annotations

import math
import re
import threading
from collections import Counter, defaultdict
from typing import Callable, Dict, Iterable, List, Optional, Tuple

_TOKEN_RE = re.compile(r"[a-z0-9]+")

STOPWORDS = frozenset("""
a an and are as at be but by for from has have he her his i in is it its my
not of on or she that the their them they this to was we were will with you
your
""".split())


def tokenize(text: str) -> List[str]:
    return [t for t in _TOKEN_RE.findall(text.lower())
            if t not in STOPWORDS and len(t) > 1]


class FulltextIndex:
    def __init__(self, k1: float = 1.2, b: float = 0.75):
        self.k1 = k1
        self.b = b
        self._lock = threading.RLock()
        self._postings: Dict[str, Dict[str, int]] = defaultdict(dict)  # term -> doc -> tf
        self._doc_len: Dict[str, int] = {}
        self._total_len = 0
        # called with the doc id after index() or remove() changed a
        # document, under the lock (search/bm25_device.py follows them)
        self._change_hooks: List[Callable[[str], None]] = []

    def __len__(self):
        return len(self._doc_len)

    def index(self, doc_id: str, text: str) -> None:
        with self._lock:
            self._remove(doc_id)
            toks = tokenize(text or "")
            if toks:
                tf = Counter(toks)
                for term, c in tf.items():
                    self._postings[term][doc_id] = c
                self._doc_len[doc_id] = len(toks)
                self._total_len += len(toks)
            self._changed(doc_id)

    def remove(self, doc_id: str) -> None:
        with self._lock:
            if self._remove(doc_id):
                self._changed(doc_id)

    def _remove(self, doc_id: str) -> bool:
        old = self._doc_len.pop(doc_id, None)
        if old is None:
            return False
        self._total_len -= old
        for term in list(self._postings):
            self._postings[term].pop(doc_id, None)
            if not self._postings[term]:
                del self._postings[term]
        return True

    def _changed(self, doc_id: str) -> None:
        for hook in self._change_hooks:
            hook(doc_id)

    @staticmethod
    def idf(n_docs: int, df: int) -> float:
        return math.log(1 + (n_docs - df + 0.5) / (df + 0.5))

    def score_terms(self, terms: Iterable[str],
                    docs: Optional[Iterable[str]] = None) -> Dict[str, float]:
        """BM25 score of every document that holds one of `terms` (one
        entry per query token, repeats count), from the statistics of the
        index as it is now; with `docs`, of those documents only. The
        caller holds the lock."""
        n_docs = len(self._doc_len)
        scores: Dict[str, float] = defaultdict(float)
        if n_docs == 0:
            return scores
        avg_len = self._total_len / n_docs
        docs = None if docs is None else list(docs)
        for term in terms:
            posting = self._postings.get(term)
            if not posting:
                continue
            idf = self.idf(n_docs, len(posting))
            if docs is None:
                items = posting.items()
            else:
                items = [(d, posting[d]) for d in docs if d in posting]
            for doc, tf in items:
                dl = self._doc_len[doc]
                s = idf * (tf * (self.k1 + 1)) / (
                    tf + self.k1 * (1 - self.b + self.b * dl / avg_len))
                scores[doc] += s
        return scores

    def search(self, query: str, k: int = 10) -> List[Tuple[str, float]]:
        with self._lock:
            if not self._doc_len:
                return []
            scores = self.score_terms(tokenize(query))
            best = sorted(scores.items(), key=lambda kv: -kv[1])
            return best[:k]

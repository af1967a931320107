"""BM25 scoring over device-resident postings.

Postings are a CSR over term ids (`BM25Postings`): the slot numbers of the
documents that hold term t are `post_doc[post_off[t]:post_off[t + 1]]`,
strictly ascending, `post_tf` their term frequencies, `doc_len[slot]` a
document's length. A query is T columns of (term id, weight); an id outside
[0, V) is skipped, and an id used in two columns counts twice. A posting
contributes

    w * tf / (tf + c0 + c1 * doc_len[slot]),  c0 = k1 (1 - b),
                                              c1 = k1 b / avg_len

and a document's score is the sum over the columns in column order. Only
documents that at least one term touched (score > 0) are hits, however few
documents match; unfilled slots are (-inf, -1).

Routes:
- GPU, k <= 64: the fused HIP kernel `bm25_scan` (csrc/bm25_scan.hip);
- GPU, larger k: a torch route that scatters the contributions into a dense
  fp32 [Q, n] in term order (`index_add_`) and takes the top-k;
- CPU: `bm25_search_exact`, which sums in float64 and is also the numerics
  oracle.

Parity: reference pkg/search/fulltext_index.go scores host maps; here the
postings live on the device.
"""

from dataclasses import dataclass
from typing import Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import native_or_none, require_native
from .knn import _NEG_INF, _mask_rows, _mask_words, _pad_unfilled

BM25_MAX_K = 64  # largest top-k list compiled into bm25_scan


@dataclass(frozen=True)
class BM25Postings:
    post_off: torch.Tensor   # int64 [V + 1]
    post_doc: torch.Tensor   # int32 [M], ascending inside a term's slice
    post_tf: torch.Tensor    # int32 [M]
    doc_len: torch.Tensor    # int32 [n_docs]
    n_docs: int

    @property
    def n_terms(self) -> int:
        return self.post_off.shape[0] - 1


def bm25_build_postings(term_docs: Sequence[Mapping[int, int]],
                        doc_len: Sequence[int], device=None) -> BM25Postings:
    """term_docs[t] maps slot -> tf for term id t; doc_len[slot] is the
    document's length. Stable sort by (term, slot)."""
    n = len(doc_len)
    assert n < 2 ** 31
    counts = np.fromiter((len(d) for d in term_docs), dtype=np.int64,
                         count=len(term_docs))
    m = int(counts.sum())
    terms = np.repeat(np.arange(len(term_docs), dtype=np.int64), counts)
    slots = np.fromiter((s for d in term_docs for s in d), dtype=np.int64,
                        count=m)
    tfs = np.fromiter((c for d in term_docs for c in d.values()),
                      dtype=np.int64, count=m)
    assert m == 0 or (slots.min() >= 0 and slots.max() < n)
    order = np.lexsort((slots, terms))   # stable; terms are already grouped
    off = np.zeros(len(term_docs) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    dev = torch.device(device or "cpu")
    return BM25Postings(
        torch.from_numpy(off).to(dev),
        torch.from_numpy(slots[order].astype(np.int32)).to(dev),
        torch.from_numpy(tfs[order].astype(np.int32)).to(dev),
        torch.as_tensor(np.asarray(doc_len, dtype=np.int32)).to(dev), n)


def _f32(x) -> float:
    """x as the kernel sees it: rounded to fp32."""
    return float(np.float32(x))


def _contributions(p: BM25Postings, q_terms, q_w, c0, c1, dtype):
    """Yields (query row, docs int64, contribution `dtype`) per valid
    (query, column), in column order. w, c0 and c1 are the fp32 values."""
    off = p.post_off.tolist()
    terms = q_terms.tolist()
    w = q_w.float()
    c0, c1 = _f32(c0), _f32(c1)
    for t in range(q_terms.shape[1]):
        for r in range(q_terms.shape[0]):
            term = terms[r][t]
            if not 0 <= term < p.n_terms or off[term + 1] <= off[term]:
                continue
            sl = slice(off[term], off[term + 1])
            docs = p.post_doc[sl].long()
            tf = p.post_tf[sl].to(dtype)
            dl = p.doc_len[docs].to(dtype)
            yield r, docs, w[r, t].to(dtype) * tf / (tf + c0 + c1 * dl)


def _dense_topk(p, q_terms, q_w, c0, c1, k, allow, dtype):
    """Dense [Q, n] scores in `dtype`, summed in column order, then the
    top-k over the touched, allowed documents."""
    n, q_count = p.n_docs, q_terms.shape[0]
    dev = p.doc_len.device
    out_s = torch.full((q_count, k), _NEG_INF, device=dev)
    out_i = torch.full((q_count, k), -1, dtype=torch.int64, device=dev)
    kk = min(k, n)
    if kk == 0:
        return out_s, out_i
    scores = torch.zeros(q_count, n, dtype=dtype, device=dev)
    for r, docs, contrib in _contributions(p, q_terms, q_w, c0, c1, dtype):
        # a term names a document once: no two adds meet
        scores[r].index_add_(0, docs, contrib)
    ok = scores > 0
    if allow is not None:
        ok &= _mask_rows(allow, 0, n)[None, :]
    s, i = torch.topk(scores.masked_fill(~ok, _NEG_INF), kk, dim=-1)
    out_s[:, :kk] = s.float()
    out_i[:, :kk] = i.masked_fill(s == _NEG_INF, -1)
    return out_s, out_i


def bm25_search_exact(
    p: BM25Postings, q_terms: torch.Tensor, q_w: torch.Tensor, c0: float,
    c1: float, k: int, allow: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Oracle and CPU path: sums in float64 from the fp32 q_w, c0 and c1
    the kernel gets. Returns (scores [Q, k] fp32, slots [Q, k] int64);
    unfilled slots are (-inf, -1)."""
    return _dense_topk(p, q_terms, q_w, c0, c1, k, allow, torch.float64)


def bm25_search(
    p: BM25Postings, q_terms: torch.Tensor, q_w: torch.Tensor, c0: float,
    c1: float, k: int, allow: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k BM25 search of the queries (q_terms int [Q, T], q_w [Q, T])
    over the postings.

    allow: optional bool [n_docs] or packed int32 slot mask on the postings'
    device. Returns (scores [Q, k] fp32, slots [Q, k] int64), descending;
    slots beyond the touched, allowed documents are (-inf, -1)."""
    assert q_terms.dim() == 2 and q_w.shape == q_terms.shape
    assert k >= 1
    dev = p.doc_len.device
    assert q_terms.device == dev and q_w.device == dev
    if allow is not None:
        assert allow.device == dev, "allow mask must live on the postings' device"
    if not p.doc_len.is_cuda:
        return bm25_search_exact(p, q_terms, q_w, c0, c1, k, allow)
    nat = native_or_none()
    if nat is None:
        require_native()  # raises: no eager fallback on GPU
    if k > BM25_MAX_K:
        return _dense_topk(p, q_terms, q_w, c0, c1, k, allow, torch.float32)
    words = None if allow is None else _mask_words(allow, p.n_docs)
    s, i = nat.bm25_scan(p.post_off, p.post_doc, p.post_tf, p.doc_len,
                         q_terms.to(torch.int32).contiguous(),
                         q_w.float().contiguous(), float(c0), float(c1), k,
                         words)
    return _pad_unfilled(s, i)

"""IVF (inverted-file) search over a local shard: score only the rows of
the probed k-means lists instead of the whole corpus.

The corpus stays in slot order. An inverted list is a CSR slice of slot
numbers (`IVFLists.list_rows[list_off[c]:list_off[c + 1]]`), all below
`n_built`; rows `[tail_start, N)` were appended after the lists were built
and are scanned by every query as one extra pseudo-list.

Routes (`ivf_route_kind`), on the GPU with D % 128 == 0 and k <= 64:
- bf16: the fused HIP kernel `ivf_scan` (csrc/ivf_scan.hip) gathers,
  scores and top-k's the probed rows;
- int8 with per-row scales: `ivf_scan_i8`, the same kernel on 1-byte rows (exact int32 dot * sa[row] * sq[query]); the query is
  quantised in torch first, as `knn_search_int8` does;
- fp8 e4m3: `ivf_scan_fp8`, fp32 accumulation of the converted bytes;
- GPU otherwise (fp32 corpora, odd D, larger k): a torch gather fallback
  (index_select of the candidate rows, matmul, top-k);
- CPU: `ivf_search_exact`, which is also the numerics oracle.

Probes of one query are a set: -1 (or any id outside [0, C)) skips, and a
list named twice is scanned once. The allow mask has the format and the
padding contract of filtered `knn_search`: unfilled slots are (-inf, -1).

Parity: reference pkg/search/kmeans_candidate_gen.go
(ClusterIndex.SearchWithClusters) routes a query to its nearest clusters
and scores their members on the host; here the lists live on the device.
"""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import native_or_none, require_native
from .knn import (_NEG_INF, _mask_rows, _mask_words, _pad_unfilled,
                  quantize_int8)

IVF_MAX_K = 64  # largest top-k list compiled into ivf_scan


@dataclass(frozen=True)
class IVFLists:
    centroids: torch.Tensor   # fp32 [C, D]
    list_off: torch.Tensor    # int32 [C + 1]
    list_rows: torch.Tensor   # int32 [M], slot numbers < n_built
    n_built: int              # rows [0, n_built) were clustered
    max_len: int              # longest list
    cnorm2: Optional[torch.Tensor] = None   # fp32 [C] |c|^2, for routing

    @property
    def n_lists(self) -> int:
        return self.list_off.shape[0] - 1


def ivf_build_lists(assign: torch.Tensor, n_clusters: int, n_built: int,
                    centroids: torch.Tensor) -> IVFLists:
    """Stable counting sort of rows [0, n_built) by cluster.

    assign[r] is row r's cluster, or -1 for a row that goes in no list
    (a tombstone). Rows keep their order inside a list."""
    assert assign.dim() == 1 and assign.shape[0] == n_built
    assert centroids.dim() == 2 and centroids.shape[0] == n_clusters
    assert n_built < 2 ** 31
    a = assign.to(torch.int64)
    assert n_built == 0 or (int(a.min()) >= -1 and int(a.max()) < n_clusters)
    member = a >= 0
    # stable sort by cluster, unlisted rows last
    order = torch.sort(torch.where(member, a, n_clusters), stable=True).indices
    m = int(member.sum())
    rows = order[:m]
    counts = torch.bincount(a[member], minlength=n_clusters)
    off = torch.zeros(n_clusters + 1, dtype=torch.int64, device=a.device)
    off[1:] = torch.cumsum(counts, 0)
    assert int(off[-1]) == m == rows.shape[0]
    assert m == 0 or (int(rows.min()) >= 0 and int(rows.max()) < n_built)
    max_len = int(counts.max()) if n_clusters > 0 else 0
    cent = centroids.float().contiguous()
    return IVFLists(cent, off.to(torch.int32).contiguous(),
                    rows.to(torch.int32).contiguous(), int(n_built), max_len,
                    (cent * cent).sum(-1))


def ivf_route(lists: IVFLists, q: torch.Tensor, nprobe: int) -> torch.Tensor:
    """int32 [Q, min(nprobe, C)]: each query's nearest centroids by squared
    L2 distance (top-k of 2 q.c - |c|^2), in fp32 torch on the data's device
    so the CPU and GPU paths pick identical probes."""
    c = lists.centroids
    cn = lists.cnorm2 if lists.cnorm2 is not None else (c * c).sum(-1)
    qf = q.float().to(c.device)
    score = torch.addmm(cn, qf, c.T, beta=-1.0, alpha=2.0)
    return torch.topk(score, min(nprobe, c.shape[0]), dim=-1) \
        .indices.to(torch.int32)


def ivf_route_kind(dtype: torch.dtype, d: int, k: int) -> str:
    """Which GPU route scores a corpus of this dtype, row width and top-k:
    "scan" (bf16), "scan_i8", "scan_fp8" (the fused kernels) or "gather"
    (the torch fallback)."""
    if d % 128 != 0 or k > IVF_MAX_K:
        return "gather"
    return {torch.bfloat16: "scan", torch.int8: "scan_i8",
            torch.float8_e4m3fn: "scan_fp8"}.get(dtype, "gather")


def _query_values(db, q):
    """fp32 query as the kNN routes of db's dtype score it."""
    if db.dtype == torch.int8:
        qi, sq = quantize_int8(q)
        return qi.float() * sq[:, None]
    if db.dtype == torch.float8_e4m3fn:
        return q.to(torch.float8_e4m3fn).float()
    return q.float()


def _row_values(rows, scales):
    return rows.float() if scales is None else rows.float() * scales[:, None]


def _reachable(lists: IVFLists, probes, n: int, tail_start: int):
    """bool [Q, n]: row in a probed list (and below tail_start) or in the
    tail."""
    c = lists.n_lists
    dev = lists.list_rows.device
    lens = (lists.list_off[1:] - lists.list_off[:-1]).to(torch.int64)
    row_list = torch.full((n,), c, dtype=torch.int64, device=dev)
    row_list[lists.list_rows.long()] = torch.repeat_interleave(
        torch.arange(c, device=dev), lens)
    p = probes.to(torch.int64)
    valid = (p >= 0) & (p < c)
    hit = torch.zeros(p.shape[0], c + 1, dtype=torch.bool, device=dev)
    hit.scatter_(1, torch.where(valid, p, c), valid)
    hit[:, c] = False
    reach = hit[:, row_list]
    reach[:, tail_start:] = True
    return reach


def ivf_search_exact(
    db: torch.Tensor, q: torch.Tensor, k: int, lists: IVFLists,
    probes: torch.Tensor, tail_start: int, row_base: int = 0,
    allow: Optional[torch.Tensor] = None,
    scales: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 oracle and CPU path: exact top-k over {rows of the probed
    lists} U tail, intersected with allow. Returns (scores [Q, k] fp32,
    indices [Q, k] int64) with k capped at N; unfilled slots (-inf, -1)."""
    n = db.shape[0]
    k = min(k, n)
    ok = _reachable(lists, probes, n, tail_start)
    if allow is not None:
        ok &= _mask_rows(allow, 0, n)[None, :]
    scores = _query_values(db, q) @ _row_values(db, scales).T
    s, i = torch.topk(scores.masked_fill(~ok, _NEG_INF), k, dim=-1)
    i = (i + row_base).masked_fill(s == _NEG_INF, -1)
    return s, i


def _candidate_rows(lists: IVFLists, probes, n: int, tail_start: int):
    """int64 [Q, L] slot numbers of every query's candidates, -1 padded.
    L = P * max_len + tail length is a bound known without a device sync."""
    c = lists.n_lists
    dev = probes.device
    p = probes.to(torch.int64)
    valid = (p >= 0) & (p < c)
    if p.shape[1] > 1:   # a list named twice is scanned once
        same = p[:, :, None] == p[:, None, :]
        valid &= ~torch.tril(same, -1).any(-1)
    pc = torch.where(valid, p, 0)
    off = lists.list_off.to(torch.int64)
    lens = torch.where(valid, off[pc + 1] - off[pc], 0)        # [Q, P]
    cum = torch.cumsum(lens, 1)
    width = p.shape[1] * lists.max_len
    j = torch.arange(width, device=dev)[None, :].expand(p.shape[0], -1)
    if width > 0:
        which = torch.searchsorted(cum, j.contiguous(), right=True)
        inside = which < p.shape[1]
        which = which.clamp_max(p.shape[1] - 1)
        start = torch.gather(cum - lens, 1, which)
        entry = torch.gather(off[pc], 1, which) + (j - start)
        entry = torch.where(inside, entry, 0)
        rows = lists.list_rows.long()[entry] if lists.list_rows.numel() \
            else torch.zeros_like(entry)
        rows = torch.where(inside & (rows < tail_start), rows, -1)
    else:
        rows = torch.empty(p.shape[0], 0, dtype=torch.int64, device=dev)
    tail = torch.arange(tail_start, n, device=dev)[None, :] \
        .expand(p.shape[0], -1)
    return torch.cat([rows, tail], 1)


def _ivf_gather(db, q, k, lists, probes, tail_start, row_base, allow, scales,
                budget_bytes: int = 256 << 20):
    """Torch gather fallback: index_select the candidate rows, score them
    with one batched matmul and take the top-k. Queries are chunked so the
    gathered block stays under budget_bytes."""
    n, d = db.shape
    qv = _query_values(db, q)
    cand = _candidate_rows(lists, probes, n, tail_start)       # [Q, L]
    width = cand.shape[1]
    kk = min(k, width)
    out_s = torch.full((q.shape[0], k), _NEG_INF, device=db.device)
    out_i = torch.full((q.shape[0], k), -1, dtype=torch.int64,
                       device=db.device)
    if kk == 0:
        return out_s, out_i
    okrow = None if allow is None else _mask_rows(allow, 0, n)
    step = max(1, budget_bytes // max(1, width * d * 4))
    for s0 in range(0, q.shape[0], step):
        cr = cand[s0:s0 + step]
        ok = cr >= 0
        flat = cr.clamp_min(0).reshape(-1)
        if okrow is not None:
            ok &= okrow[flat].view_as(cr)
        if db.dtype == torch.float8_e4m3fn:   # gather fp8 through its bytes
            rows = db.view(torch.uint8).index_select(0, flat).view(db.dtype)
        else:
            rows = db.index_select(0, flat)
        vals = _row_values(rows, None if scales is None else scales[flat])
        sc = torch.bmm(vals.view(cr.shape[0], width, d),
                       qv[s0:s0 + step, :, None]).squeeze(-1)
        s, sel = torch.topk(sc.masked_fill(~ok, _NEG_INF), kk, dim=-1)
        i = torch.gather(cr, 1, sel) + row_base
        out_s[s0:s0 + step, :kk] = s
        out_i[s0:s0 + step, :kk] = i.masked_fill(s == _NEG_INF, -1)
    return out_s, out_i


def ivf_search(
    db: torch.Tensor, q: torch.Tensor, k: int, lists: IVFLists,
    probes: torch.Tensor, tail_start: int, row_base: int = 0,
    allow: Optional[torch.Tensor] = None,
    scales: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k inner-product search of q (Q x D) over the rows of db (N x D)
    that the probed lists and the tail name.

    probes: int [Q, P] list ids per query (ivf_route), -1 = skip.
    tail_start: rows [tail_start, N) are in no list and always scanned.
    allow: optional bool [N] or packed int32 row mask on db's device.
    scales: per-row scales of an int8 corpus (quantize_int8).
    Returns (scores [Q, k] fp32, global indices [Q, k] int64), k capped at
    N; slots beyond the reachable rows are (-inf, -1)."""
    assert db.dim() == 2 and q.dim() == 2 and db.shape[1] == q.shape[1]
    assert probes.dim() == 2 and probes.shape[0] == q.shape[0]
    assert 0 <= tail_start <= db.shape[0]
    assert (db.dtype == torch.int8) == (scales is not None), \
        "int8 corpora (and only they) come with per-row scales"
    n = db.shape[0]
    k = min(k, n)
    if allow is not None:
        assert allow.device == db.device, "allow mask must live on db's device"
    if not db.is_cuda:
        return ivf_search_exact(db, q, k, lists, probes, tail_start,
                                row_base, allow, scales)
    nat = native_or_none()
    if nat is None:
        require_native()  # raises: no eager fallback on GPU
    kind = ivf_route_kind(db.dtype, db.shape[1], k)
    if kind == "gather":
        return _ivf_gather(db, q, k, lists, probes, tail_start, row_base,
                           allow, scales)
    words = None if allow is None else _mask_words(allow, n)
    tail = (probes.to(torch.int32).contiguous(), lists.list_off,
            lists.list_rows, tail_start, lists.max_len, row_base, k, words)
    if kind == "scan":
        s, i = nat.ivf_scan(db.contiguous(),
                            q.to(torch.bfloat16).contiguous(), *tail)
    elif kind == "scan_i8":
        # the query is quantised here, as in knn_search_int8, so every
        # route scores identical values
        qi, sq = quantize_int8(q)
        s, i = nat.ivf_scan_i8(db.contiguous(), scales.float().contiguous(),
                               qi.contiguous(), sq.contiguous(), *tail)
    else:
        qb = q.to(torch.float8_e4m3fn).contiguous().view(torch.uint8)
        s, i = nat.ivf_scan_fp8(db.contiguous().view(torch.uint8), qb, *tail)
    return _pad_unfilled(s, i)

"""Brute-force kNN (cosine / inner-product) over a local shard.

Replaces the reference's GPU scoring path (pkg/gpu/gpu.go:1224 EmbeddingIndex
+ pkg/gpu/cuda/cuda_kernels.cu cosine/topk kernels, which score with one
thread per vector and a <<<1,1>>> top-k). Here:

- small query batches (Q <= 16): fused HIP kernel `knn_gemv` — wave-per-row
  short8 vector loads, per-lane register top-k, one read of the shard total;
- large query batches (Q 9..256, k <= 10): fused MFMA score+top-k kernel
  (320x256 tile: 8 waves as two 160-row groups on one staged query tile,
  1 WG/CU, pipelined LDS-DMA stages, swizzled LDS; csrc/knn_mfma.hip);
- CPU: exact fp32 torch reference (also the numerics oracle for GPU tests).

Filtered search: every entry point takes an optional `allow` row mask that
the kernels test before a score can enter the top-k (see pack_allow_mask).

Scores are inner products — callers are expected to store L2-normalized
vectors for cosine semantics (same contract as the reference,
pkg/gpu/gpu.go normalized EmbeddingIndex).

Row bias: knn_search and knn_search_exact take an optional fp32 `row_bias`
[N]; the score of row r is then q.x_r + row_bias[r] on every route (one fp32
add behind the finished dot product, fused into both bf16 kernels). With
row_bias = -|x_r|^2 / 2 the ranking is the Euclidean one; that is how
EmbeddingIndex(metric="euclidean") searches.
"""

from typing import Optional, Tuple

import torch

from . import native_or_none, require_native


def _knn_bm() -> int:
    """Panel row count compiled into the kernel: KNN_RG row groups of KNN_BM
    rows, 2 x 160 = 320 by default. Shards shorter than one panel do not
    take the kernel route; rows past the last full panel are the tail."""
    nat = native_or_none()
    return int(getattr(nat, "KNN_BM", 96)) if nat is not None else 96


def _knn_q8_bm() -> int:
    """Panel row count of the quantised (int8 / fp8) kernel, 96: the same
    role as _knn_bm for csrc/knn_q8.hip."""
    nat = native_or_none()
    return int(getattr(nat, "KNN_Q8_BM", 96)) if nat is not None else 96


_NEG_INF = float("-inf")
_QMAX = 256  # query columns of one MFMA kernel launch


def pack_allow_mask(allow: torch.Tensor) -> torch.Tensor:
    """bool [N] -> int32 [ceil(N/32)] on the same device.

    Bit (r & 31) of word (r >> 5) is set when local row r (before row_base)
    may be returned. Bits at positions >= N of the last word are don't-care:
    no kernel or fallback acts on them."""
    assert allow.dim() == 1 and allow.dtype == torch.bool
    n = allow.shape[0]
    w = (n + 31) // 32
    bits = torch.zeros(w * 32, dtype=torch.uint8, device=allow.device)
    bits[:n] = allow
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8,
                           device=allow.device)
    # 8 rows -> one byte (byte arithmetic only: 1 B/row of traffic), then 4
    # bytes -> one little-endian word, byte b holding rows 8b .. 8b+7
    packed = (bits.view(w * 4, 8) * weights).sum(dim=-1, dtype=torch.uint8)
    return packed.view(torch.int32)


def unpack_allow_mask(words: torch.Tensor, n: int) -> torch.Tensor:
    """Inverse of pack_allow_mask: int32 words -> bool [n]."""
    assert words.dim() == 1 and words.dtype == torch.int32
    assert words.shape[0] * 32 >= n
    sh = torch.arange(32, device=words.device)
    bits = (words.to(torch.int64)[:, None] >> sh) & 1
    return bits.reshape(-1)[:n].bool()


def _mask_words(allow: torch.Tensor, n: int) -> torch.Tensor:
    """Caller's mask (bool [N] or packed int32) -> packed int32 words."""
    if allow.dtype == torch.bool:
        assert allow.shape == (n,), "bool allow mask must be [N]"
        return pack_allow_mask(allow)
    assert allow.dtype == torch.int32 and allow.dim() == 1 and \
        allow.shape[0] * 32 >= n, "allow must be bool [N] or int32 [ceil(N/32)]"
    return allow.contiguous()


def _mask_rows(allow: torch.Tensor, start: int, stop: int) -> torch.Tensor:
    """bool [stop-start] for local rows start..stop of either mask form."""
    if allow.dtype == torch.bool:
        return allow[start:stop]
    w0 = start >> 5
    sub = unpack_allow_mask(allow[w0:(stop + 31) >> 5], stop - w0 * 32)
    return sub[start - w0 * 32:]


def _masked_topk(scores, ok, kk, base):
    """top-kk of scores [Q, rows] over the rows with ok set; disallowed
    picks come back as (-inf, -1), everything else shifted by base."""
    if ok is not None:
        scores = scores.masked_fill(~ok, _NEG_INF)
    s, i = torch.topk(scores, kk, dim=-1)
    i = i + base
    if ok is not None:
        i = i.masked_fill(s == _NEG_INF, -1)
    return s, i


def _pad_unfilled(s, i):
    """Filtered contract: unfilled slots are (-inf, -1). The kernels leave
    their -1e30 sentinel with index -1."""
    return s.masked_fill(i < 0, _NEG_INF), i


def _merge_topk(best, new, k):
    """Running best (scores, ids), (None, None) at the start, merged with
    another row range's top-k."""
    if best[0] is None:
        return new
    cs = torch.cat([best[0], new[0]], dim=-1)
    ci = torch.cat([best[1], new[1]], dim=-1)
    s, sel = torch.topk(cs, min(k, cs.shape[-1]), dim=-1)
    return s, torch.gather(ci, -1, sel)


def _chunked_topk(score_rows, n, k, row_base, allow, chunk_rows=4 << 20,
                  start=0, best=(None, None)):
    """top-k over rows [start, n) in torch, chunk_rows at a time, on top of
    `best`. score_rows(a, b) returns the fp32 scores [Q, b - a] of rows
    a..b."""
    for a in range(start, n, chunk_rows):
        b = min(a + chunk_rows, n)
        ok = None if allow is None else _mask_rows(allow, a, b)
        top = _masked_topk(score_rows(a, b), ok, min(k, b - a), row_base + a)
        best = _merge_topk(best, top, k)
    return best


def _by_query_batches(search, q):
    """search(q) for up to _QMAX queries; larger batches (multi-GPU
    all-gather) go through it _QMAX queries at a time."""
    if q.shape[0] <= _QMAX:
        return search(q)
    parts = [search(q[s:s + _QMAX]) for s in range(0, q.shape[0], _QMAX)]
    return (torch.cat([p[0] for p in parts], 0),
            torch.cat([p[1] for p in parts], 0))


def _pad_queries(x):
    """Zero rows up to the _QMAX the MFMA kernels take."""
    if x.shape[0] == _QMAX:
        return x
    pad = torch.zeros(_QMAX - x.shape[0], *x.shape[1:], dtype=x.dtype,
                      device=x.device)
    return torch.cat([x, pad])


def knn_search_exact(
    db: torch.Tensor, q: torch.Tensor, k: int, row_base: int = 0,
    allow: Optional[torch.Tensor] = None,
    row_bias: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 exact reference: returns (scores [Q,k] fp32, indices [Q,k] int64)."""
    scores = q.float() @ db.float().T
    if row_bias is not None:
        scores = scores + row_bias.float()
    ok = None if allow is None else _mask_rows(allow, 0, db.shape[0])
    return _masked_topk(scores, ok, k, row_base)


def _knn_gemm_chunked(
    db: torch.Tensor, q: torch.Tensor, k: int, row_base: int,
    chunk_rows: int = 4 << 20, allow: Optional[torch.Tensor] = None,
    row_bias: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Tiled GEMM + top-k. Avoids materializing the full [N, Q] score matrix.

    With a row bias the product is taken in fp32, in chunks small enough for
    an fp32 copy: a bf16 GEMM rounds its output to 8 bits, and q.x + bias
    cancels (a Euclidean bias is -|x|^2/2 against q.x of the same size)."""
    qf = q.to(db.dtype)
    if row_bias is not None:
        chunk_rows = min(chunk_rows, 1 << 18)
        qf = q.float()

    def score_rows(start, stop):
        if row_bias is None:
            return (qf @ db[start:stop].T).float()  # [Q, chunk]
        return qf @ db[start:stop].float().T + row_bias[start:stop]

    return _chunked_topk(score_rows, db.shape[0], k, row_base, allow,
                         chunk_rows)


def _check_row_bias(row_bias: torch.Tensor, db: torch.Tensor) -> torch.Tensor:
    """Caller's bias -> contiguous fp32 [N] on db's device, or ValueError."""
    if db.dtype not in (torch.bfloat16, torch.float32, torch.float16):
        raise ValueError(
            "row_bias is supported on bf16/float corpora only, not "
            f"{db.dtype}: metrics on quantised corpora are not implemented")
    if row_bias.dim() != 1 or row_bias.shape[0] != db.shape[0]:
        raise ValueError(
            f"row_bias must be [N] = [{db.shape[0]}], got {tuple(row_bias.shape)}")
    if row_bias.device != db.device:
        raise ValueError("row_bias must live on db's device")
    return row_bias.float().contiguous()


def knn_search(
    db: torch.Tensor, q: torch.Tensor, k: int, row_base: int = 0,
    allow: Optional[torch.Tensor] = None,
    row_bias: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k inner-product search of q (Q x D) against db (N x D).

    db may be bf16 or float8_e4m3fn (opt-in quantized corpus — half the
    HBM traffic, 2x capacity; scored by the fp8 MFMA kernel on GPU).
    Returns (scores [Q,k] fp32, global indices [Q,k] int64).

    allow: optional row filter shared by all queries — a bool [N] tensor or
    a packed int32 mask (pack_allow_mask) on db's device. With m allowed
    rows the first min(k, m) slots hold the allowed top scores in
    descending order; every remaining slot is (score -inf, index -1).

    row_bias: optional fp32 [N] on db's device, indexed like the mask by
    local row (before row_base). Scores become q.x + row_bias[row] on every
    route; `allow` and `row_bias` combine. Values must be finite and far
    above -1e30, the kernels' empty-slot sentinel (not tested). Raises
    ValueError on a quantised (fp8) corpus.
    """
    assert db.dim() == 2 and q.dim() == 2 and db.shape[1] == q.shape[1]
    k = min(k, db.shape[0])
    if row_bias is not None:
        row_bias = _check_row_bias(row_bias, db)
    if allow is None:
        return _knn_dispatch(db, q, k, row_base, None, row_bias)
    assert allow.device == db.device, "allow mask must live on db's device"
    if db.is_cuda:
        allow = _mask_words(allow, db.shape[0])
    return _pad_unfilled(*_knn_dispatch(db, q, k, row_base, allow, row_bias))


def _knn_dispatch(db, q, k, row_base, allow, row_bias=None):
    """Q/k/dtype routing; allow is None or (on GPU) packed mask words,
    row_bias None or contiguous fp32 [N] (never with an fp8 corpus)."""
    if not db.is_cuda:
        return knn_search_exact(db, q, k, row_base, allow, row_bias)
    if db.dtype == torch.float8_e4m3fn:
        nat = native_or_none()
        if nat is None:
            require_native()
        if (k <= 10 and db.shape[1] % 128 == 0
                and db.shape[0] >= _knn_q8_bm()):
            return _by_query_batches(
                lambda qq: _knn_fp8(nat, db, qq, k, row_base, allow), q)
        return _knn_fp8_chunked(db, q, k, row_base, allow=allow)

    nat = native_or_none()
    if nat is None:
        require_native()  # raises: no eager fallback on GPU
    # Crossover measured on MI355X (4M x 1024): gemv wins to Q=8
    # (3.8 TB/s @ Q=1, 2.3 TB/s @ Q=8); for Q>8 the padded fused-MFMA
    # kernel is faster than the dot2 gemv (4.0 ms vs 7.1 ms @ Q=16).
    if (
        q.shape[0] <= 8
        and k <= 16
        and db.dtype == torch.bfloat16
        and db.shape[1] % 128 == 0
    ):
        qq = q.to(torch.bfloat16).contiguous()
        return nat.knn_gemv(db.contiguous(), qq, row_base, k, allow, row_bias)
    if (
        k <= 10
        and db.dtype == torch.bfloat16
        and db.shape[1] % 64 == 0
        and db.shape[0] >= _knn_bm()
    ):
        return _by_query_batches(
            lambda qq: _knn_mfma(nat, db, qq, k, row_base, allow, row_bias), q)
    if (
        q.shape[0] <= 16
        and k <= 16
        and db.dtype == torch.bfloat16
        and db.shape[1] % 128 == 0
    ):
        # Q 9..16 with k 11..16: MFMA path capped at k<=10, gemv still wins
        # over the chunked-GEMM fallback at these batch sizes
        qq = q.to(torch.bfloat16).contiguous()
        return nat.knn_gemv(db.contiguous(), qq, row_base, k, allow, row_bias)
    return _knn_gemm_chunked(db, q, k, row_base, allow=allow,
                             row_bias=row_bias)


def quantize_fp8(db: torch.Tensor) -> torch.Tensor:
    """bf16/f32 rows -> OCP float8_e4m3fn (the gfx950 fp8 MFMA format)."""
    return db.to(torch.float8_e4m3fn)


def quantize_int8(db: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetric per-row int8: returns (int8 [N,D], fp32 scales [N]).

    ~7 effective bits on normalized vectors (vs e4m3's 3-bit mantissa) —
    the recommended quantized-corpus format; scored by the gfx950 i8
    MFMA at 2x the bf16 rate."""
    f = db.float()
    scale = f.abs().amax(dim=-1).clamp_min(1e-12) / 127.0
    q = torch.round(f / scale[:, None]).clamp(-127, 127).to(torch.int8)
    return q, scale


def knn_search_int8(
    db: torch.Tensor, sa: torch.Tensor, q: torch.Tensor, k: int,
    row_base: int = 0, allow: Optional[torch.Tensor] = None,
    row_bias: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k over a symmetric int8 corpus (per-row scales sa).

    q is float (bf16/f32); it is int8-quantized internally so GPU main
    panels and the tail score identical values. i32 dots are exact in
    fp32 up to d*127^2 < 2^24 (d <= 1024).

    allow: optional row filter, same forms and contract as knn_search.
    row_bias: not supported on a quantised corpus; anything but None raises
    ValueError."""
    assert db.dtype == torch.int8 and db.dim() == 2
    if row_bias is not None:
        raise ValueError("row_bias is not supported on an int8 corpus: "
                         "metrics on quantised corpora are not implemented")
    k = min(k, db.shape[0])
    if allow is None:
        return _knn_int8_dispatch(db, sa, q, k, row_base, None)
    assert allow.device == db.device, "allow mask must live on db's device"
    if db.is_cuda:
        allow = _mask_words(allow, db.shape[0])
    return _pad_unfilled(*_knn_int8_dispatch(db, sa, q, k, row_base, allow))


def _knn_int8_dispatch(db, sa, q, k, row_base, allow):
    if not db.is_cuda:
        qi, sq = quantize_int8(q)
        scores = (qi.float() * sq[:, None]) @ (db.float() * sa[:, None]).T
        ok = None if allow is None else _mask_rows(allow, 0, db.shape[0])
        return _masked_topk(scores, ok, k, row_base)
    nat = native_or_none()
    if nat is None:
        require_native()
    if k <= 10 and db.shape[1] % 128 == 0 and db.shape[0] >= _knn_q8_bm():
        return _by_query_batches(
            lambda qq: _knn_int8(nat, db, sa, qq, k, row_base, allow), q)
    # k > 10 / odd dims: chunked dequantized scoring
    qi, sq = quantize_int8(q)
    qf = (qi.float() * sq[:, None]).to(torch.bfloat16)

    def score_rows(start, stop):
        chunk = (db[start:stop].float() * sa[start:stop, None]).to(torch.bfloat16)
        return (qf @ chunk.T).float()

    return _chunked_topk(score_rows, db.shape[0], k, row_base, allow)


def _knn_int8(nat, db, sa, q, k, row_base, allow=None):
    """Fused i8 MFMA score+topk over full panels + torch-scored tail, both
    on the int8-quantised q."""
    qn = q.shape[0]
    qi, sq = quantize_int8(q)
    n = db.shape[0]
    n_main = (n // _knn_q8_bm()) * _knn_q8_bm()
    s, i = nat.knn_i8(db.narrow(0, 0, n_main).contiguous(),
                      sa.narrow(0, 0, n_main).contiguous().float(),
                      _pad_queries(qi).contiguous(),
                      _pad_queries(sq).contiguous().float(),
                      row_base, k, allow)
    qd = qi.float() * sq[:, None]
    return _chunked_topk(
        lambda a, b: qd @ (db[a:b].float() * sa[a:b, None]).T,
        n, k, row_base, allow, start=n_main, best=(s[:qn], i[:qn]))


def _knn_fp8(nat, db, q, k, row_base, allow=None):
    """Fused fp8 MFMA score+topk over full panels + torch tail.

    q is quantized to e4m3fn so main-panel and tail scores agree
    (both score the same representable values)."""
    qn = q.shape[0]
    q8 = q.to(torch.float8_e4m3fn)
    qu = _pad_queries(q8).contiguous().view(torch.uint8)
    n = db.shape[0]
    n_main = (n // _knn_q8_bm()) * _knn_q8_bm()
    s, i = nat.knn_fp8(db.narrow(0, 0, n_main).view(torch.uint8), qu,
                       row_base, k, allow)
    qb = q8.to(torch.bfloat16)
    return _chunked_topk(
        lambda a, b: (qb @ db[a:b].to(torch.bfloat16).T).float(),
        n, k, row_base, allow, start=n_main, best=(s[:qn], i[:qn]))


def _knn_fp8_chunked(db, q, k, row_base, chunk_rows: int = 4 << 20,
                     allow=None):
    """Dequantize-per-chunk fallback (k > 10 or odd dims)."""
    qf = q.to(torch.bfloat16)
    return _chunked_topk(
        lambda a, b: (qf @ db[a:b].to(torch.bfloat16).T).float(),
        db.shape[0], k, row_base, allow, chunk_rows)


def _knn_mfma(nat, db, q, k, row_base, allow=None, row_bias=None):
    """Fused MFMA score+topk over full BM-row panels + torch-scored tail."""
    qn = q.shape[0]
    qb = q.to(torch.bfloat16)
    n = db.shape[0]
    bm = _knn_bm()
    n_main = (n // bm) * bm
    s, i = nat.knn_mfma(
        db.narrow(0, 0, n_main), _pad_queries(qb).contiguous(), row_base, k,
        allow, None if row_bias is None else row_bias.narrow(0, 0, n_main), qn)

    def score_tail(a, b):
        if row_bias is None:
            return (qb @ db[a:b].T).float()
        # fp32 product: the bf16 GEMM's rounded output would not survive
        # the cancellation against the bias
        return qb.float() @ db[a:b].float().T + row_bias[a:b]

    return _chunked_topk(score_tail, n, k, row_base, allow, start=n_main,
                         best=(s[:qn], i[:qn]))

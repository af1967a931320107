// IVF probe-list scan for NornicDB-AMD: fused gather + score + per-block
// top-K over the probed inverted lists, for bf16, int8 and fp8 corpora, and
// its host code. Selection itself (register lists, cross-block merge) is
// topk.h.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "common.h"
#include "allow_mask.h"
#include "topk.h"

// ---------------------------------------------------------------------------
// IVF probe-list scan: fused gather + cosine-score + per-block top-K.
//
// The corpus stays in slot order; an inverted list is a CSR slice of slot
// numbers (list_rows[list_off[c] .. list_off[c+1])). One 256-thread block
// serves one (query, probe, split) triple: it stages its query in LDS and
// its 16 lane-groups stride through the list's entries, each group scoring
// one gathered row per step with the gemv kernel's dot product (a row is
// contiguous, so every 16-lane load is still fully coalesced).
// Probe slot n_probe is the tail pseudo-list: rows [tail_start, n) with
// the identity mapping, scanned by every query.
//
// After the butterfly every lane of a group holds the same score, so all
// 16 lanes run the same register insert and the block ends with 16 sorted
// K-lists. They go to LDS and each of the 16*K entries finds its rank in
// the union by a binary search in every list (ties broken by position, so
// ranks are a permutation); ranks < K are written out. That leaves ONE
// candidate list per block for topk_merge(), in its [W][Q][K] layout with
// W = p_eff * split.
//
// A probe outside [0, n_lists), or equal to an earlier probe of the same
// query, scans nothing. List entries are accepted only when they name a
// row below tail_start, so no row is scored twice or read out of bounds.
// FILTERED tests the allow bit before the row is loaded (allow_mask.h).
// ---------------------------------------------------------------------------

// A block's split, probe slot and query; block-uniform.
struct IvfBlock {
  int sp, p, q;
};

DEV_INLINE IvfBlock ivf_block(int p_eff, int split) {
  IvfBlock b;
  b.sp = blockIdx.x % split;
  b.p = (blockIdx.x / split) % p_eff;
  b.q = blockIdx.x / (split * p_eff);
  return b;
}

// The entries [begin, end) of a block's list; block-uniform. An empty range
// means there is nothing to scan. The kernel calls this behind its query
// staging loop: the dependent scalar loads (probe, then list offsets) then
// run behind the staging loads instead of in front of them, which measured
// ~1 us per call on the quantised scans.
struct IvfRange {
  bool tail;
  long long begin, end;
  unsigned int row_limit;  // entries must name a row below this
};

DEV_INLINE IvfRange ivf_list_range(const IvfBlock& b,
                                   const int* __restrict__ probes,
                                   const int* __restrict__ list_off,
                                   int n_lists, long long n_entries,
                                   int n_probe, int tail_start, int n) {
  IvfRange r;
  r.tail = (b.p == n_probe);
  r.begin = 0;
  r.end = 0;
  if (r.tail) {
    r.begin = tail_start;
    r.end = n;
  } else {
    const int* pq = probes + (long long)b.q * n_probe;
    const int c = pq[b.p];
    if (c >= 0 && c < n_lists) {
      bool dup = false;
      for (int j = 0; j < b.p; ++j) dup |= (pq[j] == c);
      if (!dup) {
        r.begin = max(list_off[c], 0);
        r.end = min((long long)list_off[c + 1], n_entries);
      }
    }
  }
  r.row_limit = r.tail ? (unsigned int)n : (unsigned int)tail_start;
  return r;
}

// The block's 16 sorted K-lists (one per lane group g16, identical in the
// group's 16 lanes) go to LDS; every entry finds its rank in their union and
// ranks < K are written to the block's candidate list at out_base. Contains
// a __syncthreads(): every thread of the block calls it.
template <int K>
DEV_INLINE void ivf_rank_merge(const float (&tv)[K], const int (&ti)[K],
                               int g16, int gl, float* s_ls, int* s_li,
                               long long out_base, long long row_base,
                               float* __restrict__ cand_score,
                               long long* __restrict__ cand_idx) {
  if (gl == 0) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      s_ls[g16 * K + i] = tv[i];
      s_li[g16 * K + i] = ti[i];
    }
  }
  __syncthreads();

  for (int x = threadIdx.x; x < 16 * K; x += blockDim.x) {
    const float xs = s_ls[x];
    int rank = 0;
#pragma unroll 4
    for (int l = 0; l < 16; ++l) {
      const float* ls = s_ls + l * K;
      const int pos0 = l * K;
      int lo = 0;
#pragma unroll
      for (int step = K / 2; step >= 1; step >>= 1) {
        const int j = lo + step - 1;
        const float a = ls[j];
        lo += (a > xs || (a == xs && pos0 + j < x)) ? step : 0;
      }
      const float a = ls[lo];
      lo += (a > xs || (a == xs && pos0 + lo < x)) ? 1 : 0;
      rank += lo;
    }
    if (rank < K) {
      const int r = s_li[x];
      cand_score[out_base + rank] = xs;
      cand_idx[out_base + rank] = r < 0 ? -1LL : row_base + (long long)r;
    }
  }
}

// ---------------------------------------------------------------------------
// The row score, the one part of the scan that depends on the corpus format.
// Per 128 elements each of a group's 16 lanes loads 8 of the row's (rp) and
// 8 of the query's from LDS (qp); both pointers are the lane's own, nj =
// d / 128. Every format ends with the same 16-lane butterfly, after which
// all 16 lanes hold the score.
//
// bf16: v_dot2 accumulates pairs into fp32.
// int8: the query arrives quantised (int8 [Q][d] and its scale sq[q]);
//   v_dot4 accumulates into an int32 that the butterfly reduces exactly,
//   score = float(dot) * sa[row] * sq[q] as in k_knn_q8.
// fp8: row and query bytes are converted in pairs (v_cvt_pk_f32_fp8, exact)
//   and accumulated in fp32.
// row_scale and q_scale are used by int8 alone.
// ---------------------------------------------------------------------------
template <int FMT>
DEV_INLINE float ivf_row_score(const unsigned char* rp,
                               const unsigned char* qp, int nj,
                               float row_scale, float q_scale) {
  if constexpr (FMT == Q8_FMT_BF16) {
    float acc = 0.0f;
#pragma unroll 8
    for (int jj = 0; jj < nj; ++jj) {
      short8v v = *reinterpret_cast<const short8v*>(rp + jj * 256);
      short8v qv = *reinterpret_cast<const short8v*>(qp + jj * 256);
      const bf16x2v* xa = reinterpret_cast<const bf16x2v*>(&v);
      const bf16x2v* qa = reinterpret_cast<const bf16x2v*>(&qv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc = __builtin_amdgcn_fdot2_f32_bf16(xa[j], qa[j], acc, false);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      acc += __shfl_xor(acc, off, WAVE);
    return acc;
  } else if constexpr (FMT == Q8_FMT_I8) {
    int acc = 0;
#pragma unroll 8
    for (int jj = 0; jj < nj; ++jj) {
      uint2v v = *reinterpret_cast<const uint2v*>(rp + jj * 128);
      uint2v qv = *reinterpret_cast<const uint2v*>(qp + jj * 128);
      acc = __builtin_amdgcn_sdot4((int)v.x, (int)qv.x, acc, false);
      acc = __builtin_amdgcn_sdot4((int)v.y, (int)qv.y, acc, false);
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      acc += __shfl_xor(acc, off, WAVE);
    return (float)acc * row_scale * q_scale;
  } else {
    float acc = 0.0f;
#pragma unroll 8
    for (int jj = 0; jj < nj; ++jj) {
      uint2v v = *reinterpret_cast<const uint2v*>(rp + jj * 128);
      uint2v qv = *reinterpret_cast<const uint2v*>(qp + jj * 128);
      const unsigned int xw[2] = {v.x, v.y}, qw[2] = {qv.x, qv.y};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float2v x0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)xw[j], false);
        float2v x1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)xw[j], true);
        float2v q0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)qw[j], false);
        float2v q1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)qw[j], true);
        acc = fmaf(x0.x, q0.x, acc);
        acc = fmaf(x0.y, q0.y, acc);
        acc = fmaf(x1.x, q1.x, acc);
        acc = fmaf(x1.y, q1.y, acc);
      }
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
      acc += __shfl_xor(acc, off, WAVE);
    return acc;
  }
}

// FMT: Q8_FMT_BF16, Q8_FMT_I8 or Q8_FMT_FP8. db [n][d] and qs [q_count][d]
// are addressed in bytes; sa (fp32 [n], indexed by slot number) and sq
// (fp32 [q_count]) are read by int8 alone and may be null otherwise.
// Dynamic LDS: the query, d elements, then the 16 K-lists of ivf_rank_merge.
template <int K, bool FILTERED, int FMT>
__global__ void __launch_bounds__(256)
k_ivf_scan(const unsigned char* __restrict__ db,
           const unsigned char* __restrict__ qs,
           const float* __restrict__ sa,
           const float* __restrict__ sq,
           const int* __restrict__ probes,
           const int* __restrict__ list_off,
           const int* __restrict__ list_rows,
           int n_lists, long long n_entries, int n_probe, int p_eff,
           int split, int tail_start, int n, int d, int q_count,
           long long row_base,
           float* __restrict__ cand_score,
           long long* __restrict__ cand_idx,
           const unsigned int* __restrict__ allow) {
  constexpr int ELEM = (FMT == Q8_FMT_BF16) ? 2 : 1;  // bytes per element
  // 8 elements, one lane's share of a 128-element step
  using Chunk = std::conditional_t<FMT == Q8_FMT_BF16, short8v, uint2v>;

  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  unsigned char* s_q = s_raw;                                        // [d]
  float* s_ls = reinterpret_cast<float*>(s_raw + (size_t)d * ELEM);  // [16][K]
  int* s_li = reinterpret_cast<int*>(s_ls + 16 * K);                 // [16][K]

  const int lane = threadIdx.x & (WAVE - 1);
  const int grp = lane >> 4;
  const int gl = lane & 15;
  const int wid = threadIdx.x / WAVE;
  const int g16 = wid * 4 + grp;    // lane-group within the block, 0..15

  const IvfBlock blk = ivf_block(p_eff, split);
  const int sp = blk.sp, p = blk.p, q = blk.q;

  for (int i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
    *reinterpret_cast<Chunk*>(s_q + i * ELEM) =
        *reinterpret_cast<const Chunk*>(qs + ((long long)q * d + i) * ELEM);
  }
  float q_scale = 1.0f;
  if constexpr (FMT == Q8_FMT_I8) q_scale = sq[q];
  const IvfRange rng = ivf_list_range(blk, probes, list_off, n_lists, n_entries,
                                      n_probe, tail_start, n);
  const bool tail = rng.tail;
  const long long begin = rng.begin, end = rng.end;
  const unsigned int row_limit = rng.row_limit;
  __syncthreads();

  float tv[K];
  int ti[K];
  topk_init(tv, ti);

  const int nj = d / 128;
  const long long stride = (long long)split * 16;
  long long e = begin + sp * 16 + g16;
  int row = -1;
  if (e < end) row = tail ? (int)e : list_rows[e];
  while (e < end) {
    // next entry's slot number is fetched before this row is scored
    const long long e_next = e + stride;
    int row_next = -1;
    if (e_next < end) row_next = tail ? (int)e_next : list_rows[e_next];

    bool ok = (unsigned int)row < row_limit;
    if constexpr (FILTERED) {
      if (ok) ok = (allow[row >> 5] >> (row & 31)) & 1u;
    }
    if (ok) {
      // its own cache line per row: in flight with the row's data
      float row_scale = 1.0f;
      if constexpr (FMT == Q8_FMT_I8) row_scale = sa[row];
      const float score = ivf_row_score<FMT>(
          db + ((long long)row * d + gl * 8) * ELEM, s_q + gl * 8 * ELEM, nj,
          row_scale, q_scale);
      // same score in all 16 lanes of the group: uniform insert
      if (score > tv[K - 1]) topk_insert(tv, ti, score, row);
    }
    e = e_next;
    row = row_next;
  }

  // rank of every entry in the union of the 16 sorted lists
  const long long out_base =
      (((long long)p * split + sp) * q_count + q) * K;
  ivf_rank_merge(tv, ti, g16, gl, s_ls, s_li, out_base, row_base, cand_score,
                 cand_idx);
}

// ===========================================================================
// Host wrappers
// ===========================================================================

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------------
// IVF scan + merge. probes [Q][P] int32 (any value outside [0, C) skips);
// list_off [C+1] / list_rows [M] int32 CSR of slot numbers below tail_start;
// rows [tail_start, N) are scanned by every query. max_len is the longest
// list, recorded when the lists were built (no device sync per search).
// ivf_scan (bf16), ivf_scan_i8 and ivf_scan_fp8 share the argument checks,
// the grid, the launch and the merge; they differ in the corpus / query
// dtype and in the kernel's FMT.
// ---------------------------------------------------------------------------
struct IvfPlan {
  int n, d, qc, n_probe, p_eff, split, tail_start, k_out;
  long long row_base;
  const unsigned int* allow_p;
};

// Validates the arguments every IVF scan takes and sizes the grid. A
// p_eff of 0 means there is nothing to scan.
static IvfPlan ivf_scan_plan(const char* who, const at::Tensor& db,
                             at::ScalarType db_type, const char* db_name,
                             const at::Tensor& q, at::ScalarType q_type,
                             const at::Tensor& probes,
                             const at::Tensor& list_off,
                             const at::Tensor& list_rows, long long tail_start,
                             long long max_len, long long row_base, int k_out,
                             const c10::optional<at::Tensor>& allow) {
  TORCH_CHECK(db.is_cuda() && db.dim() == 2 && db.is_contiguous() &&
                  db.scalar_type() == db_type,
              who, ": db must be contiguous 2D ", db_name, " CUDA");
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.is_contiguous() &&
                  q.scalar_type() == q_type,
              who, ": q must be contiguous 2D ", db_name, " CUDA");
  for (const at::Tensor* t : {&probes, &list_off, &list_rows})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == at::kInt,
                who, ": probes, list_off and list_rows must be contiguous "
                "int32 CUDA tensors");
  TORCH_CHECK(q.device() == db.device() && probes.device() == db.device() &&
                  list_off.device() == db.device() &&
                  list_rows.device() == db.device(),
              who, ": all tensors must be on db's device");
  const long long n = db.size(0);
  const int d = (int)db.size(1);
  const long long qc = q.size(0);
  TORCH_CHECK(q.size(1) == d, who, ": dim mismatch");
  TORCH_CHECK(d % 128 == 0, who, " needs D % 128 == 0");
  TORCH_CHECK(n <= 0x7fffffffLL, who, ": int32 slot numbers, N < 2^31");
  TORCH_CHECK(qc >= 1, who, ": need at least one query");
  TORCH_CHECK(probes.dim() == 2 && probes.size(0) == qc,
              who, ": probes must be [Q, P]");
  TORCH_CHECK(list_off.dim() == 1 && list_off.numel() >= 1 &&
                  list_rows.dim() == 1,
              who, ": list_off must be [C+1] and list_rows [M]");
  TORCH_CHECK(tail_start >= 0 && tail_start <= n,
              who, ": tail_start must be in [0, N]");
  TORCH_CHECK(max_len >= 0, who, ": max_len must be >= 0");
  TORCH_CHECK(k_out >= 1 && k_out <= 64, who, ": k_out must be in 1..64");
  const unsigned int* allow_p = nullptr;
  if (allow.has_value()) allow_p = check_allow_mask(*allow, db, n, who);

  const long long n_probe = probes.size(1);
  const long long tail_len = n - tail_start;
  const long long p_eff = n_probe + (tail_len > 0 ? 1 : 0);

  // ~4 blocks per CU over the whole grid, but every split of the longest
  // list keeps at least block_rows rows: each block adds one candidate
  // list to the merge, which costs more than the rows it would take over
  // (4M x 1024, Q=1, nprobe=8: 74 us at 16 rows, 42 us at 128, 49 at 256)
  int block_rows = 128;
  if (const char* g = getenv("NORNICDB_IVF_BLOCK_ROWS"))
    block_rows = std::max(atoi(g), 1);
  const long long longest = std::max<long long>(std::max(max_len, tail_len), 1);
  long long split = 1;
  if (p_eff > 0) {
    split = std::max<long long>(1024 / (qc * p_eff), 1);
    split = std::min(split, (longest + block_rows - 1) / block_rows);
    TORCH_CHECK(qc * p_eff * split <= 0x7fffffffLL, who, ": grid too large");
  }
  return {(int)n, d, (int)qc, (int)n_probe, (int)p_eff, (int)split,
          (int)tail_start, k_out, row_base, allow_p};
}

static std::tuple<at::Tensor, at::Tensor> ivf_nothing_to_scan(
    const IvfPlan& pl, const at::Tensor& db) {
  return {at::full({pl.qc, pl.k_out}, -1e30f, db.options().dtype(at::kFloat)),
          at::full({pl.qc, pl.k_out}, -1LL, db.options().dtype(at::kLong))};
}

// Allocates the [W][Q][K] candidates, launches the scan over them and merges
// them into [Q][k_out]. sa / sq are null unless FMT is int8.
template <int K, int FMT>
static std::tuple<at::Tensor, at::Tensor> ivf_scan_run(
    const char* who, const IvfPlan& pl, const at::Tensor& db,
    const at::Tensor& q, const float* sa, const float* sq,
    const at::Tensor& probes, const at::Tensor& list_off,
    const at::Tensor& list_rows) {
  auto opts_f = db.options().dtype(at::kFloat);
  auto opts_i = db.options().dtype(at::kLong);
  const long long w = (long long)pl.p_eff * pl.split;
  at::Tensor out_s = at::empty({pl.qc, pl.k_out}, opts_f);
  at::Tensor out_i = at::empty({pl.qc, pl.k_out}, opts_i);
  at::Tensor cand_s = at::empty({w, pl.qc, K}, opts_f);
  at::Tensor cand_i = at::empty({w, pl.qc, K}, opts_i);
  const size_t q_bytes = (size_t)pl.d * (FMT == Q8_FMT_BF16 ? 2 : 1);
  const size_t lds = q_bytes + (size_t)16 * K * 8;
  TORCH_CHECK(lds <= 64 * 1024, who, ": D too large for the LDS query tile");
  auto kern = pl.allow_p ? k_ivf_scan<K, true, FMT> : k_ivf_scan<K, false, FMT>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(w * pl.qc)), dim3(256), lds,
                     cur_stream(), (const unsigned char*)db.data_ptr(),
                     (const unsigned char*)q.data_ptr(), sa, sq,
                     probes.data_ptr<int>(), list_off.data_ptr<int>(),
                     list_rows.data_ptr<int>(), (int)list_off.numel() - 1,
                     (long long)list_rows.numel(), pl.n_probe, pl.p_eff,
                     pl.split, pl.tail_start, pl.n, pl.d, pl.qc, pl.row_base,
                     cand_s.data_ptr<float>(),
                     reinterpret_cast<long long*>(cand_i.data_ptr<int64_t>()),
                     pl.allow_p);
  HIP_CHECK_LAST();
  // the scan added row_base to its ids
  topk_merge(cand_s, cand_i, w, pl.qc, pl.k_out, 0, out_s, out_i,
             cur_stream());
  return {out_s, out_i};
}

std::tuple<at::Tensor, at::Tensor> ivf_scan(
    at::Tensor db, at::Tensor q, at::Tensor probes, at::Tensor list_off,
    at::Tensor list_rows, long long tail_start, long long max_len,
    long long row_base, int k_out, c10::optional<at::Tensor> allow) {
  const char* who = "ivf_scan";
  const IvfPlan pl = ivf_scan_plan(who, db, at::kBFloat16, "bf16", q,
                                   at::kBFloat16, probes, list_off, list_rows,
                                   tail_start, max_len, row_base, k_out, allow);
  if (pl.p_eff == 0) return ivf_nothing_to_scan(pl, db);
  if (k_out <= 16)
    return ivf_scan_run<16, Q8_FMT_BF16>(who, pl, db, q, nullptr, nullptr,
                                         probes, list_off, list_rows);
  return ivf_scan_run<64, Q8_FMT_BF16>(who, pl, db, q, nullptr, nullptr,
                                       probes, list_off, list_rows);
}

std::tuple<at::Tensor, at::Tensor> ivf_scan_i8(
    at::Tensor db, at::Tensor sa, at::Tensor q, at::Tensor sq,
    at::Tensor probes, at::Tensor list_off, at::Tensor list_rows,
    long long tail_start, long long max_len, long long row_base, int k_out,
    c10::optional<at::Tensor> allow) {
  const char* who = "ivf_scan_i8";
  const IvfPlan pl = ivf_scan_plan(who, db, at::kChar, "int8", q, at::kChar,
                                   probes, list_off, list_rows, tail_start,
                                   max_len, row_base, k_out, allow);
  for (const at::Tensor* t : {&sa, &sq})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == at::kFloat &&
                    t->device() == db.device(),
                who, ": sa and sq must be contiguous fp32 tensors on db's "
                "device");
  TORCH_CHECK(sa.numel() == pl.n, who, ": sa must hold one scale per row, N");
  TORCH_CHECK(sq.numel() == pl.qc, who,
              ": sq must hold one scale per query, Q");
  if (pl.p_eff == 0) return ivf_nothing_to_scan(pl, db);
  const float* sap = sa.data_ptr<float>();
  const float* sqp = sq.data_ptr<float>();
  if (k_out <= 16)
    return ivf_scan_run<16, Q8_FMT_I8>(who, pl, db, q, sap, sqp, probes,
                                       list_off, list_rows);
  return ivf_scan_run<64, Q8_FMT_I8>(who, pl, db, q, sap, sqp, probes,
                                     list_off, list_rows);
}

std::tuple<at::Tensor, at::Tensor> ivf_scan_fp8(
    at::Tensor db, at::Tensor q, at::Tensor probes, at::Tensor list_off,
    at::Tensor list_rows, long long tail_start, long long max_len,
    long long row_base, int k_out, c10::optional<at::Tensor> allow) {
  const char* who = "ivf_scan_fp8";
  const IvfPlan pl = ivf_scan_plan(who, db, at::kByte, "uint8 (e4m3 bytes)", q,
                                   at::kByte, probes, list_off, list_rows,
                                   tail_start, max_len, row_base, k_out,
                                   allow);
  if (pl.p_eff == 0) return ivf_nothing_to_scan(pl, db);
  if (k_out <= 16)
    return ivf_scan_run<16, Q8_FMT_FP8>(who, pl, db, q, nullptr, nullptr,
                                        probes, list_off, list_rows);
  return ivf_scan_run<64, Q8_FMT_FP8>(who, pl, db, q, nullptr, nullptr,
                                      probes, list_off, list_rows);
}

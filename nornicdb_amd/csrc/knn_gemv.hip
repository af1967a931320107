// Fused cosine-score + top-k over a bf16 corpus, GEMV path for small query
// batches (Q <= 16). Selection itself (register lists, cross-block merge)
// is topk.h.
//
// Re-designs (not ports of) the reference's CUDA kernels
// (reference: pkg/gpu/cuda/cuda_kernels.cu:185-460 — 1-thread-per-vector
// scoring and a <<<1,1>>> top-k): the kernel is wave64-shaped,
// vector-loaded (short8 = 8 x bf16 per lane) and fused so the embedding
// matrix is read exactly once per query batch.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "allow_mask.h"
#include "topk.h"

// ---------------------------------------------------------------------------
// Fused cosine-score + per-block top-k, GEMV path (Q <= 16).
//
// Each 16-LANE GROUP owns one DB row (4 rows per wave in flight), so the
// cross-lane reduction is 4 shfl steps instead of 6 and a wave retires 4
// rows per iteration. Lane g*16+l covers elements [l*64, l*64+64) of the
// row (8 x short8 loads = 128 B/lane, 2 KB contiguous per group). After
// the 16-lane reduce, lane l of the group holds score(row, q=l) and folds
// it into a per-(group, q) register top-K list (statically unrolled
// insert). Candidates land in cand[group_global][q][K].
//
// Queries are staged in LDS as bf16.
//
// FILTERED: `allow` is a packed row mask (allow_mask.h). A group tests its
// row's bit before touching the row and skips a disallowed row without
// loading it, so a selective filter saves HBM traffic in proportion. All
// 16 lanes of a group share the row and take the same branch; the
// __shfl_xor offsets (< 16) never leave the group.
//
// BIASED: the score that enters the top-k is dot(q, row) + row_bias[row],
// row_bias fp32 [n] indexed like the mask (local row, before row_base). The
// group's bias load is issued ahead of the row's loads (its own cache line,
// in flight with the row's data, as sa[row] in k_ivf_scan) and added
// once, in fp32, after the 16-lane butterfly has completed the dot product.
// Biases must be finite and far above the -1e30 list sentinel; the kernel
// does not test for that. BIASED=false never touches `row_bias`.
// ---------------------------------------------------------------------------
template <int QMAX, int K, bool FILTERED, bool BIASED>
__global__ void k_knn_gemv_bf16(const unsigned short* __restrict__ db,
                                const unsigned short* __restrict__ qs,
                                long long n, int d, int q_count,
                                long long row_base,
                                float* __restrict__ cand_score,
                                long long* __restrict__ cand_idx,
                                const unsigned int* __restrict__ allow,
                                const float* __restrict__ row_bias) {
  extern __shared__ unsigned short s_q[];  // [q_count][d]
  const int lane = threadIdx.x & (WAVE - 1);
  const int grp = lane >> 4;        // 4 row-groups per wave
  const int gl = lane & 15;         // lane within group
  const int wid = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;

  // stage queries
  for (int i = threadIdx.x * 8; i < q_count * d; i += blockDim.x * 8) {
    *reinterpret_cast<short8v*>(s_q + i) =
        *reinterpret_cast<const short8v*>(qs + i);
  }
  __syncthreads();

  const long long wave_global = (long long)blockIdx.x * waves_per_block + wid;
  const long long total_waves = (long long)gridDim.x * waves_per_block;
  const long long group_global = wave_global * 4 + grp;
  const long long total_groups = total_waves * 4;
  const int nj = d / 128;           // 16 lanes x 8 elems per j-step

  // private top-K (valid in lane gl == q for q < q_count)
  float tv[K];
  long long ti[K];
  topk_init(tv, ti);

  for (long long row = group_global; row < n; row += total_groups) {
    if constexpr (FILTERED) {
      if (!((allow[row >> 5] >> (row & 31)) & 1u)) continue;
    }
    float rb = 0.0f;
    if constexpr (BIASED) rb = row_bias[row];
    const unsigned short* rp = db + row * d + (long long)gl * 8;
    float acc[QMAX];
#pragma unroll
    for (int q = 0; q < QMAX; ++q) acc[q] = 0.0f;

    // lane gl reads elems [jj*128 + gl*8 .. +8): 16 lanes cover a
    // contiguous 256 B segment per step (coalesced)
#pragma unroll 4
    for (int jj = 0; jj < nj; ++jj) {
      short8v v = *reinterpret_cast<const short8v*>(rp + jj * 128);
      const bf16x2v* xa = reinterpret_cast<const bf16x2v*>(&v);
#pragma unroll
      for (int q = 0; q < QMAX; ++q) {
        if (q >= q_count) break;
        short8v qv = *reinterpret_cast<const short8v*>(
            s_q + q * d + jj * 128 + gl * 8);
        const bf16x2v* qa = reinterpret_cast<const bf16x2v*>(&qv);
        // v_dot2c_f32_bf16: 2 bf16 MACs/instr, f32 accumulate — no
        // explicit converts, 4 instrs per 8 elems per query
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[q] = __builtin_amdgcn_fdot2_f32_bf16(xa[j], qa[j], acc[q], false);
      }
    }
    // reduce each query's partials across the 16-lane group
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
      if (q >= q_count) break;
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        acc[q] += __shfl_xor(acc[q], off, WAVE);
    }
    // lane gl keeps the score for query gl
    if (gl < q_count) {
      float s = acc[0];
#pragma unroll
      for (int q = 1; q < QMAX; ++q)
        if (gl == q) s = acc[q];
      if constexpr (BIASED) s += rb;
      if (s > tv[K - 1]) topk_insert(tv, ti, s, row_base + row);
    }
  }

  if (gl < q_count) {
    long long base = (group_global * q_count + gl) * K;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      cand_score[base + i] = tv[i];
      cand_idx[base + i] = ti[i];
    }
  }
}

// ===========================================================================
// Host wrapper
// ===========================================================================

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

constexpr int KNN_K = 16;

std::tuple<at::Tensor, at::Tensor> knn_gemv(at::Tensor db, at::Tensor q,
                                            long long row_base, int k_out,
                                            c10::optional<at::Tensor> allow,
                                            c10::optional<at::Tensor> row_bias) {
  TORCH_CHECK(db.is_cuda() && db.dim() == 2 && db.is_contiguous() &&
                  db.scalar_type() == at::kBFloat16,
              "knn_gemv: db must be contiguous 2D bf16 CUDA");
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.is_contiguous() &&
                  q.scalar_type() == at::kBFloat16,
              "knn_gemv: q must be contiguous 2D bf16 CUDA");
  long long n = db.size(0);
  int d = (int)db.size(1);
  int qc = (int)q.size(0);
  TORCH_CHECK(q.size(1) == d, "dim mismatch");
  TORCH_CHECK(qc >= 1 && qc <= 16, "knn_gemv supports 1..16 queries");
  TORCH_CHECK(d % 128 == 0, "knn_gemv needs D % 128 == 0");
  TORCH_CHECK(k_out >= 1 && k_out <= KNN_K, "k_out must be <= ", KNN_K);
  const unsigned int* allow_p = nullptr;
  if (allow.has_value()) allow_p = check_allow_mask(*allow, db, n, "knn_gemv");
  const float* bias_p = nullptr;
  if (row_bias.has_value())
    bias_p = check_row_bias(*row_bias, db, n, "knn_gemv");

  int cap = 1280;
  if (const char* g = getenv("NORNICDB_GEMV_BLOCKS")) cap = atoi(g);
  int blocks = (int)std::min<long long>((n + 1023) / 1024, cap);
  blocks = std::max(blocks, 1);
  long long waves = (long long)blocks * 4 * 4;  // 4 waves x 4 row-groups

  auto opts_f = db.options().dtype(at::kFloat);
  auto opts_i = db.options().dtype(at::kLong);
  at::Tensor cand_s = at::empty({waves, qc, KNN_K}, opts_f);
  at::Tensor cand_i = at::empty({waves, qc, KNN_K}, opts_i);
  size_t lds = (size_t)qc * d * sizeof(unsigned short);
  TORCH_CHECK(lds <= 64 * 1024, "query LDS tile too large");

  auto launch =
      bias_p ? (allow_p ? k_knn_gemv_bf16<16, KNN_K, true, true>
                        : k_knn_gemv_bf16<16, KNN_K, false, true>)
             : (allow_p ? k_knn_gemv_bf16<16, KNN_K, true, false>
                        : k_knn_gemv_bf16<16, KNN_K, false, false>);
  hipLaunchKernelGGL(launch, dim3(blocks), dim3(256),
                     lds, cur_stream(), (const unsigned short*)db.data_ptr(),
                     (const unsigned short*)q.data_ptr(), n, d, qc, row_base,
                     cand_s.data_ptr<float>(), reinterpret_cast<long long*>(cand_i.data_ptr<int64_t>()),
                     allow_p, bias_p);
  HIP_CHECK_LAST();

  at::Tensor out_s = at::empty({qc, k_out}, opts_f);
  at::Tensor out_i = at::empty({qc, k_out}, opts_i);
  // candidates hold global ids already
  topk_merge(cand_s, cand_i, waves, qc, k_out, 0, out_s, out_i, cur_stream());
  return {out_s, out_i};
}

// Cross-block top-k merge: the one kernel behind topk_merge() (topk.h),
// called by knn_gemv, knn_mfma, knn_i8 / knn_fp8 and the IVF scans.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "topk.h"

// ---------------------------------------------------------------------------
// Merge per-block candidate lists into final top-k.
// cand_*: [W][q_stride][K]; one block per query; k_out rounds of packed
// argmax-reduce. Packs (monotonic_score_bits << 32 | slot) into uint64 for
// the reduce.
// Always launched with 256 threads; the bound lets K=64 keep its lists in
// registers (192 of them with int64 ids) instead of spilling at the default
// 128-VGPR cap.
// ---------------------------------------------------------------------------
template <int K, typename IDX>
__global__ void __launch_bounds__(256)
k_topk_merge(const float* __restrict__ cand_score,
             const IDX* __restrict__ cand_idx, long long w, int q_stride,
             int k_out, long long row_base, float* __restrict__ out_score,
             long long* __restrict__ out_idx) {
  const int q = blockIdx.x;
  const long long total = w * K;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  __shared__ unsigned long long s_best[8];

  // each thread scans strided candidates into a private top-K
  float tv[K];
  IDX ti[K];
  // topk_init() written out: with the helper K=64 with int64 ids needs 267
  // VGPRs and spills 18 of them, written out 227 and none
#pragma unroll
  for (int i = 0; i < K; ++i) { tv[i] = -1e30f; ti[i] = -1; }
  for (long long j = threadIdx.x; j < total; j += blockDim.x) {
    long long src = ((j / K) * q_stride + q) * K + (j % K);
    float s = cand_score[src];
    if (s > tv[K - 1]) topk_insert(tv, ti, s, cand_idx[src]);
  }

  // k_out rounds: global argmax over every thread's current head element.
  int head = 0;
  for (int r = 0; r < k_out; ++r) {
    float hv = -1e30f;
    // select current head value via static unroll (keeps tv in registers)
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i == head) hv = tv[i];
    unsigned long long packed =
        ((unsigned long long)f32_mono(hv) << 32) | (unsigned int)threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      unsigned long long o = __shfl_xor(packed, off, WAVE);
      if (o > packed) packed = o;
    }
    if (lane == 0) s_best[wid] = packed;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long b = s_best[0];
      for (int i = 1; i < (int)(blockDim.x / WAVE); ++i)
        if (s_best[i] > b) b = s_best[i];
      s_best[0] = b;
    }
    __syncthreads();
    int winner = (int)(s_best[0] & 0xffffffffu);
    if (threadIdx.x == winner) {
      float wv = -1e30f;
      IDX wi = -1;
#pragma unroll
      for (int i = 0; i < K; ++i)
        if (i == head) { wv = tv[i]; wi = ti[i]; }
      out_score[(long long)q * k_out + r] = wv;
      out_idx[(long long)q * k_out + r] = wi < 0 ? -1 : row_base + wi;
      head++;  // only the winner moves on to its next element
    }
    __syncthreads();
  }
}

template <int K, typename IDX>
static void launch_topk_merge(const at::Tensor& cand_s,
                              const at::Tensor& cand_i, long long w,
                              int q_stride, int k_out, long long row_base,
                              at::Tensor& out_s, at::Tensor& out_i,
                              hipStream_t stream) {
  hipLaunchKernelGGL(
      (k_topk_merge<K, IDX>), dim3((unsigned)out_s.size(0)), dim3(256), 0,
      stream, cand_s.data_ptr<float>(),
      reinterpret_cast<const IDX*>(cand_i.data_ptr()), w, q_stride, k_out,
      row_base, out_s.data_ptr<float>(),
      reinterpret_cast<long long*>(out_i.data_ptr<int64_t>()));
}

void topk_merge(const at::Tensor& cand_s, const at::Tensor& cand_i,
                long long w, int q_stride, int k_out, long long row_base,
                at::Tensor& out_s, at::Tensor& out_i, hipStream_t stream) {
  const long long k = cand_s.size(-1);
  TORCH_CHECK(cand_s.numel() == w * q_stride * k &&
                  cand_i.numel() == cand_s.numel() &&
                  out_s.size(0) <= q_stride && out_s.size(1) == k_out,
              "topk_merge: candidates [w, q_stride, K], outputs [Q, k_out]");
  TORCH_CHECK(k_out >= 1 && k_out <= k, "topk_merge: k_out must be in 1..K");
  const bool i32 = cand_i.scalar_type() == at::kInt;
  TORCH_CHECK(i32 || cand_i.scalar_type() == at::kLong,
              "topk_merge: candidate ids must be int32 or int64");
  auto launch = launch_topk_merge<10, int>;
  if (k == 10) launch = i32 ? launch_topk_merge<10, int>
                            : launch_topk_merge<10, long long>;
  else if (k == 16) launch = i32 ? launch_topk_merge<16, int>
                                 : launch_topk_merge<16, long long>;
  else if (k == 64) launch = i32 ? launch_topk_merge<64, int>
                                 : launch_topk_merge<64, long long>;
  else TORCH_CHECK(false, "topk_merge: K must be 10, 16 or 64, got ", k);
  launch(cand_s, cand_i, w, q_stride, k_out, row_base, out_s, out_i, stream);
  HIP_CHECK_LAST();
}

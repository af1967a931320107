// Tier-1 vector kernels for NornicDB-AMD: L2 normalize and synthetic corpus
// generation. The kNN kernels are knn_gemv.hip, knn_mfma.hip and knn_q8.hip,
// the IVF probe-list scan is ivf_scan.hip.
//
// Re-designs (not ports of) the reference's CUDA kernels
// (reference: pkg/gpu/cuda/cuda_kernels.cu:185-460 — 1-thread-per-vector
// norms): here every kernel is wave64-shaped and vector-loaded (short8 =
// 8 x bf16 per lane).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

// ---------------------------------------------------------------------------
// L2 normalize rows, in-place. bf16 [N][D], D % 8 == 0.
// One wave per row; lane l covers elements [l*8, l*8+8) striding WAVE*8.
// ---------------------------------------------------------------------------
__global__ void k_l2_normalize_bf16(unsigned short* __restrict__ x,
                                    long long n, int d, float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  const long long wave_global = (long long)blockIdx.x * waves_per_block + wid;
  const long long total_waves = (long long)gridDim.x * waves_per_block;

  for (long long row = wave_global; row < n; row += total_waves) {
    unsigned short* rp = x + row * d;
    float ss = 0.0f;
    for (int c = lane * 8; c < d; c += WAVE * 8) {
      short8v v = *reinterpret_cast<const short8v*>(rp + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_bits_to_f32((unsigned short)v[j]);
        ss += f * f;
      }
    }
    ss = wave_reduce_sum(ss);
    float inv = rsqrtf(ss + eps);
    for (int c = lane * 8; c < d; c += WAVE * 8) {
      short8v v = *reinterpret_cast<const short8v*>(rp + c);
      short8v o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_bits_to_f32((unsigned short)v[j]) * inv;
        o[j] = (short)f32_to_bf16_bits(f);
      }
      *reinterpret_cast<short8v*>(rp + c) = o;
    }
  }
}

__global__ void k_l2_normalize_f32(float* __restrict__ x, long long n, int d,
                                   float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  const long long wave_global = (long long)blockIdx.x * waves_per_block + wid;
  const long long total_waves = (long long)gridDim.x * waves_per_block;

  for (long long row = wave_global; row < n; row += total_waves) {
    float* rp = x + row * d;
    float ss = 0.0f;
    for (int c = lane * 4; c < d; c += WAVE * 4) {
      float4v v = *reinterpret_cast<const float4v*>(rp + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) ss += v[j] * v[j];
    }
    ss = wave_reduce_sum(ss);
    float inv = rsqrtf(ss + eps);
    for (int c = lane * 4; c < d; c += WAVE * 4) {
      float4v v = *reinterpret_cast<const float4v*>(rp + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= inv;
      *reinterpret_cast<float4v*>(rp + c) = v;
    }
  }
}

// ---------------------------------------------------------------------------
// Fill rows with deterministic pseudo-gaussian values, L2-normalized.
// Used to generate benchmark corpora at HBM speed (no curand round trip).
// Row identity is (row_base + row) so multi-GPU shards are globally
// consistent and reproducible.
// ---------------------------------------------------------------------------
__global__ void k_fill_random_unit_bf16(unsigned short* __restrict__ x,
                                        long long n, int d,
                                        long long row_base,
                                        unsigned long long seed) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int waves_per_block = blockDim.x / WAVE;
  const long long wave_global = (long long)blockIdx.x * waves_per_block + wid;
  const long long total_waves = (long long)gridDim.x * waves_per_block;

  for (long long row = wave_global; row < n; row += total_waves) {
    const unsigned long long rk =
        seed ^ (0x100000001b3ULL * (unsigned long long)(row_base + row));
    float ss = 0.0f;
    // pass 1: sum of squares
    for (int c = lane * 2; c < d; c += WAVE * 2) {
      float2v g = hash_gauss2(rk + (unsigned long long)c);
      ss += g.x * g.x + g.y * g.y;
    }
    ss = wave_reduce_sum(ss);
    float inv = rsqrtf(ss + 1e-12f);
    // pass 2: regenerate, scale, store
    unsigned short* rp = x + row * d;
    for (int c = lane * 2; c < d; c += WAVE * 2) {
      float2v g = hash_gauss2(rk + (unsigned long long)c);
      unsigned int lo = f32_to_bf16_bits(g.x * inv);
      unsigned int hi = f32_to_bf16_bits(g.y * inv);
      *reinterpret_cast<unsigned int*>(rp + c) = lo | (hi << 16);
    }
  }
}

// ===========================================================================
// Host wrappers
// ===========================================================================

static inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void l2_normalize_(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous(),
              "l2_normalize_: need contiguous 2D CUDA tensor");
  long long n = x.size(0);
  int d = (int)x.size(1);
  int blocks = (int)std::min<long long>((n + 3) / 4, 8192);
  if (blocks == 0) return;
  if (x.scalar_type() == at::kBFloat16) {
    TORCH_CHECK(d % 8 == 0, "bf16 l2_normalize_ needs D % 8 == 0");
    hipLaunchKernelGGL(k_l2_normalize_bf16, dim3(blocks), dim3(256), 0,
                       cur_stream(), (unsigned short*)x.data_ptr(), n, d,
                       1e-12f);
  } else if (x.scalar_type() == at::kFloat) {
    TORCH_CHECK(d % 4 == 0, "f32 l2_normalize_ needs D % 4 == 0");
    hipLaunchKernelGGL(k_l2_normalize_f32, dim3(blocks), dim3(256), 0,
                       cur_stream(), x.data_ptr<float>(), n, d, 1e-12f);
  } else {
    TORCH_CHECK(false, "l2_normalize_: dtype must be bf16 or f32");
  }
  HIP_CHECK_LAST();
}

void fill_random_unit_(at::Tensor x, long long row_base, long long seed) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() &&
                  x.scalar_type() == at::kBFloat16,
              "fill_random_unit_: need contiguous 2D bf16 CUDA tensor");
  long long n = x.size(0);
  int d = (int)x.size(1);
  TORCH_CHECK(d % 2 == 0, "fill_random_unit_ needs D % 2 == 0");
  int blocks = (int)std::min<long long>((n + 3) / 4, 16384);
  if (blocks == 0) return;
  hipLaunchKernelGGL(k_fill_random_unit_bf16, dim3(blocks), dim3(256), 0,
                     cur_stream(), (unsigned short*)x.data_ptr(), n, d,
                     row_base, (unsigned long long)seed);
  HIP_CHECK_LAST();
}

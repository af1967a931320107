// Fused encoder ops for the bge-m3 (XLM-R) forward pass.
//
// Replaces the reference's llama.cpp/ggml encoder internals
// (reference pkg/localllm/llama.go:104-180) with hand-written CDNA4
// kernels:
//   - k_add_layernorm      : y = LN(a + b) * gamma + beta   (bf16, fp32 stats)
//   - k_bias_gelu          : y = gelu_erf(x + bias)          (bf16)
//   - k_mean_pool_l2norm   : masked mean over S + L2 norm    (bf16 -> fp32)
// (The attention kernel lives in flash_attn.hip.)
// All memory-bound kernels use short8 (16 B/lane) vector loads per the
// CDNA4 guide (G13).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

// ---------------------------------------------------------------------------
// y = LayerNorm(a + b) * gamma + beta. Rows = tokens, D % 8 == 0, D <= 8192.
// One wave per row.
// ---------------------------------------------------------------------------
__global__ void k_add_layernorm(const unsigned short* __restrict__ a,
                                const unsigned short* __restrict__ b,
                                const unsigned short* __restrict__ gamma,
                                const unsigned short* __restrict__ beta,
                                unsigned short* __restrict__ y,
                                long long rows, int d, float eps) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int wpb = blockDim.x / WAVE;
  const long long w0 = (long long)blockIdx.x * wpb + wid;
  const long long tw = (long long)gridDim.x * wpb;

  for (long long row = w0; row < rows; row += tw) {
    const unsigned short* pa = a + row * d;
    const unsigned short* pb = b ? b + row * d : nullptr;
    float sum = 0.f, sq = 0.f;
    // cache the summed row in registers: up to 8192/64 = 128 floats... too
    // many; re-read instead (L2-hot).
    for (int c = lane * 8; c < d; c += WAVE * 8) {
      short8v va = *reinterpret_cast<const short8v*>(pa + c);
      short8v vb;
      if (pb) vb = *reinterpret_cast<const short8v*>(pb + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_bits_to_f32((unsigned short)va[j]);
        if (pb) f += bf16_bits_to_f32((unsigned short)vb[j]);
        sum += f;
        sq += f * f;
      }
    }
    sum = wave_reduce_sum(sum);
    sq = wave_reduce_sum(sq);
    float mean = sum / d;
    float var = sq / d - mean * mean;
    // A row far from zero (|mean| > 2 std) loses the variance in
    // E[x^2] - mean^2, and the mean its last digits. Such a row is summed
    // again as x - x[0], and the shift is kept apart from the then small
    // mean. x - x[0] is exact where the two are within a factor of 2 of
    // each other (Sterbenz), which is where the cancellation is; elsewhere
    // it is rounded once, to 2^-24 of a difference of std size, not of mean
    // size. Every other row
    // keeps the single pass and its arithmetic. The condition is the same
    // in all lanes, is true for a negative var (NaN root), and does not
    // use mean * mean, so that the product above has one use and stays
    // fused into var.
    float shift = 0.f;
    if (!(fabsf(mean) <= 2.f * sqrtf(var))) {
      shift = bf16_bits_to_f32(pa[0]);
      if (pb) shift += bf16_bits_to_f32(pb[0]);
      sum = 0.f;
      sq = 0.f;
      for (int c = lane * 8; c < d; c += WAVE * 8) {
        short8v va = *reinterpret_cast<const short8v*>(pa + c);
        short8v vb;
        if (pb) vb = *reinterpret_cast<const short8v*>(pb + c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float f = bf16_bits_to_f32((unsigned short)va[j]);
          if (pb) f += bf16_bits_to_f32((unsigned short)vb[j]);
          f -= shift;
          sum += f;
          sq += f * f;
        }
      }
      sum = wave_reduce_sum(sum);
      sq = wave_reduce_sum(sq);
      mean = sum / d;  // of the shifted row
      var = sq / d - mean * mean;
    }
    float inv = rsqrtf(fmaxf(var, 0.f) + eps);
    unsigned short* py = y + row * d;
    for (int c = lane * 8; c < d; c += WAVE * 8) {
      short8v va = *reinterpret_cast<const short8v*>(pa + c);
      short8v vb;
      if (pb) vb = *reinterpret_cast<const short8v*>(pb + c);
      short8v vg = *reinterpret_cast<const short8v*>(gamma + c);
      short8v vbe = *reinterpret_cast<const short8v*>(beta + c);
      short8v o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = bf16_bits_to_f32((unsigned short)va[j]);
        if (pb) f += bf16_bits_to_f32((unsigned short)vb[j]);
        float g = bf16_bits_to_f32((unsigned short)vg[j]);
        float be = bf16_bits_to_f32((unsigned short)vbe[j]);
        o[j] = (short)f32_to_bf16_bits(((f - shift) - mean) * inv * g + be);
      }
      *reinterpret_cast<short8v*>(py + c) = o;
    }
  }
}

// ---------------------------------------------------------------------------
// y = gelu(x + bias), exact erf form (XLM-R GELU). x [rows][d], bias [d].
// Grid-stride elementwise, short8 vectorized.
// ---------------------------------------------------------------------------
__global__ void k_bias_gelu(const unsigned short* __restrict__ x,
                            const unsigned short* __restrict__ bias,
                            unsigned short* __restrict__ y,
                            long long total, int d) {
  long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (long long i = i0; i < total; i += stride) {
    short8v v = *reinterpret_cast<const short8v*>(x + i);
    int c = (int)(i % d);
    short8v vb = *reinterpret_cast<const short8v*>(bias + c);
    short8v o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_bits_to_f32((unsigned short)v[j]) +
                bf16_bits_to_f32((unsigned short)vb[j]);
      float g = 0.5f * f * (1.0f + erff(f * 0.70710678f));
      o[j] = (short)f32_to_bf16_bits(g);
    }
    *reinterpret_cast<short8v*>(y + i) = o;
  }
}

// ---------------------------------------------------------------------------
// Masked mean-pool over sequence + L2 normalize: x [B][S][D] bf16,
// mask [B][S] (int32, 1=real), out [B][D] fp32 unit-norm.
// One block per batch row; lanes split D.
// ---------------------------------------------------------------------------
__global__ void k_mean_pool_l2norm(const unsigned short* __restrict__ x,
                                   const int* __restrict__ mask,
                                   float* __restrict__ out,
                                   int bsz, int s, int d) {
  const int b = blockIdx.x;
  if (b >= bsz) return;
  extern __shared__ float s_acc[];  // [d]
  for (int c = threadIdx.x; c < d; c += blockDim.x) s_acc[c] = 0.f;
  __syncthreads();
  int count = 0;
  for (int t = 0; t < s; ++t) {
    if (mask && mask[b * s + t] == 0) continue;
    count++;
    const unsigned short* p = x + ((long long)b * s + t) * d;
    for (int c = threadIdx.x * 8; c < d; c += blockDim.x * 8) {
      short8v v = *reinterpret_cast<const short8v*>(p + c);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        s_acc[c + j] += bf16_bits_to_f32((unsigned short)v[j]);
    }
    __syncthreads();
  }
  // mean + norm
  float inv_n = 1.0f / max(count, 1);
  float ss = 0.f;
  for (int c = threadIdx.x; c < d; c += blockDim.x) {
    float m = s_acc[c] * inv_n;
    s_acc[c] = m;
    ss += m * m;
  }
  __shared__ float s_red[8];
  ss = block_reduce_sum(ss, s_red);
  float inv = rsqrtf(ss + 1e-12f);
  for (int c = threadIdx.x; c < d; c += blockDim.x)
    out[(long long)b * d + c] = s_acc[c] * inv;
}

// ===========================================================================
// Host wrappers
// ===========================================================================

static inline hipStream_t enc_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

at::Tensor add_layernorm(at::Tensor a, c10::optional<at::Tensor> b,
                         at::Tensor gamma, at::Tensor beta, double eps) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16);
  auto a2 = a.contiguous();
  TORCH_CHECK(a2.dim() >= 1 && a2.size(-1) > 0 && a2.size(-1) % 8 == 0 &&
                  a2.size(-1) <= 8192,
              "add_layernorm: D % 8 == 0, 0 < D <= 8192");
  long long rows = a2.numel() / a2.size(-1);
  int d = (int)a2.size(-1);
  at::Tensor y = at::empty_like(a2);
  const unsigned short* bp = nullptr;
  at::Tensor bc;
  if (b.has_value()) {
    bc = b->contiguous();
    TORCH_CHECK(bc.is_cuda() && bc.scalar_type() == at::kBFloat16 &&
                    bc.sizes() == a2.sizes(),
                "add_layernorm: b must be bf16 CUDA of a's shape");
    bp = (const unsigned short*)bc.data_ptr();
  }
  TORCH_CHECK(gamma.is_cuda() && beta.is_cuda() && gamma.numel() == d &&
                  beta.numel() == d,
              "add_layernorm: gamma and beta must be CUDA [D]");
  if (rows == 0) return y.view(a.sizes());
  auto g = gamma.contiguous().to(at::kBFloat16);
  auto be = beta.contiguous().to(at::kBFloat16);
  int blocks = (int)std::min<long long>((rows + 3) / 4, 4096);
  hipLaunchKernelGGL(k_add_layernorm, dim3(blocks), dim3(256), 0, enc_stream(),
                     (const unsigned short*)a2.data_ptr(), bp,
                     (const unsigned short*)g.data_ptr(),
                     (const unsigned short*)be.data_ptr(),
                     (unsigned short*)y.data_ptr(), rows, d, (float)eps);
  HIP_CHECK_LAST();
  return y.view(a.sizes());
}

at::Tensor bias_gelu(at::Tensor x, at::Tensor bias) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16);
  auto x2 = x.contiguous();
  TORCH_CHECK(x2.dim() >= 1 && x2.size(-1) > 0 && x2.size(-1) % 8 == 0,
              "bias_gelu: D % 8 == 0, D > 0");
  int d = (int)x2.size(-1);
  TORCH_CHECK(bias.is_cuda() && bias.numel() == d,
              "bias_gelu: bias must be CUDA [D]");
  auto b = bias.contiguous().to(at::kBFloat16);
  at::Tensor y = at::empty_like(x2);
  long long total = x2.numel();
  if (total == 0) return y.view(x.sizes());
  int blocks = (int)std::min<long long>((total / 8 + 255) / 256, 4096);
  hipLaunchKernelGGL(k_bias_gelu, dim3(blocks), dim3(256), 0, enc_stream(),
                     (const unsigned short*)x2.data_ptr(),
                     (const unsigned short*)b.data_ptr(),
                     (unsigned short*)y.data_ptr(), total, d);
  HIP_CHECK_LAST();
  return y.view(x.sizes());
}

at::Tensor mean_pool_l2norm(at::Tensor x, c10::optional<at::Tensor> mask) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3 && x.scalar_type() == at::kBFloat16);
  auto x2 = x.contiguous();
  int bsz = (int)x2.size(0), s = (int)x2.size(1), d = (int)x2.size(2);
  TORCH_CHECK(d > 0 && d % 8 == 0, "mean_pool_l2norm: D % 8 == 0, D > 0");
  const int* mp = nullptr;
  at::Tensor mc;
  if (mask.has_value()) {
    mc = mask->to(at::kInt).contiguous();
    TORCH_CHECK(mc.is_cuda() && mc.dim() == 2 && mc.size(0) == bsz &&
                    mc.size(1) == s,
                "mean_pool_l2norm: mask must be CUDA [B,S]");
    mp = mc.data_ptr<int>();
  }
  at::Tensor out = at::empty({bsz, d}, x2.options().dtype(at::kFloat));
  if (bsz == 0) return out;
  size_t lds = (size_t)d * sizeof(float);
  hipLaunchKernelGGL(k_mean_pool_l2norm, dim3(bsz), dim3(256), lds,
                     enc_stream(), (const unsigned short*)x2.data_ptr(), mp,
                     out.data_ptr<float>(), bsz, s, d);
  HIP_CHECK_LAST();
  return out;
}


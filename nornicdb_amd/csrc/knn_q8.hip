// Fused MFMA score + top-k kNN over a 1-byte-per-element corpus: k_knn_q8,
// for FP8 (OCP e4m3fn) and symmetric int8 with per-row scales.
//
// Opt-in quantized search mode: the corpus is stored at 1 B/element —
// HALF the HBM/LDS traffic of bf16 and 2x the per-GPU capacity (200M+
// 1024-d vectors in 288 GB) — scored with the gfx950 fp8 MFMA
// (mfma_f32_16x16x32_fp8_fp8; non-scaled fp8 runs at the bf16 MFMA rate,
// so the win is bandwidth, not math). Scores accumulate in fp32.
// MEASURED (8M x 1024): fp8 1.37x the bf16 kernel but recall@10 only
// 0.91 on worst-case gaussian corpora — e4m3's 3-bit mantissa is too
// coarse; the int8 variant below (per-row scales) holds 0.98 and is
// the recommended mode. The reference has no
// quantized mode (pkg/gpu scores fp32 only) — this is MI355X-native
// headroom, gated behind EmbeddingIndex(quant="fp8").
//
// The int8 variant is the same kernel (k_knn_q8<Q8_FMT_I8>): symmetric
// per-row absmax scales give ~7 effective bits (recall@10 ~0.98-0.99 even on
// worst-case gaussian corpora), and the gfx950 i8 MFMA
// (mfma_i32_16x16x64_i8, K=64/instr) runs at 2x the bf16 rate.
// score = i32_dot * sa[row] * sq[col], applied in the epilogue.
//
// Geometry: a block owns a 96-row x 256-query output tile (4 waves, one
// query quarter of 64 columns each, all 96 rows: a 6 x 4 grid of 16x16
// accumulators per wave) and walks the panels blockIdx.x, + gridDim.x, ...
// Per 128-element K tile it stages the panel's rows (96 x 128 B = 12 KB)
// and the query tile (256 x 128 B = 32 KB) with global_load_lds, 1 KB per
// wave instruction, 16 B slots XOR-swizzled by row (swz8); then
// __syncthreads(), the MFMA steps over the staged rows (8 B fragments and
// 4 k-steps of 32 for fp8, 16 B fragments and 2 k-steps of 64 for int8),
// and a second __syncthreads() before the next tile overwrites the
// buffers. There is no prefetch across tiles. The epilogue transposes the
// accumulators 32 rows at a time through a [256][36] block that aliases
// the staging buffers; each thread owns one query column and keeps a
// register top-K list (topk.h).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "common.h"
#include "allow_mask.h"
#include "topk.h"

#define G_AS __attribute__((address_space(1)))
#define L_AS __attribute__((address_space(3)))

#define F8_BM 96
#define F8_BN 256
#define F8_BK 128          // K-elements per tile (= 128 B rows)
#define F8_NTHREADS 256
#define F8_KCAND 10
#define F8_MW (F8_BM / 16)

typedef int int4v_ __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int swz8(int b) {
  return (b & ~127) | ((b & 127) ^ (((b >> 7) & 7) << 4));
}

// FMT: Q8_FMT_FP8 (db / qs are e4m3fn bytes, sa_g / sq_g unused) or
// Q8_FMT_I8 (int8 bytes; sa_g fp32 [N] row scales, sq_g fp32 [256] query
// column scales). The formats differ in the accumulator type, the MFMA and
// its fragment, and the scaling of the score in the epilogue.
// FILTERED: `allow` is a packed row mask (allow_mask.h), three whole words
// per 96-row panel. A panel whose words are all zero is skipped before
// anything is staged; the row's bit joins the insertion guard in the
// epilogue. FILTERED=false never touches `allow`.
template <int FMT, bool FILTERED>
__global__ __launch_bounds__(F8_NTHREADS, 3) void k_knn_q8(
    const unsigned char* __restrict__ db, const float* __restrict__ sa_g,
    const unsigned char* __restrict__ qs, const float* __restrict__ sq_g,
    long long n_panels, int d, long long row_base,
    float* __restrict__ cand_score, int* __restrict__ cand_idx,
    const unsigned int* __restrict__ allow) {
  static_assert(!FILTERED || F8_BM % 32 == 0,
                "filtered kNN needs whole mask words per panel");
  constexpr bool I8 = FMT == Q8_FMT_I8;
  using acc_t = std::conditional_t<I8, int4v_, float4v>;
  using elem_t = std::conditional_t<I8, int, float>;
  using frag_t = std::conditional_t<I8, int4v_, long>;  // 16 B / 8 B per lane
  constexpr int KS = I8 ? 64 : 32;                      // K of one MFMA
  // 44 KB: sA (12 KB) + sB (32 KB); epilogue aliases [256][36] accumulators.
  __shared__ __align__(16) char smem[F8_BM * F8_BK + F8_BN * F8_BK];
  char* sA = smem;
  char* sB = smem + F8_BM * F8_BK;
  elem_t* sT = (elem_t*)smem;

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wc = tid / WAVE;

  float tv[F8_KCAND];
  int ti[F8_KCAND];
  topk_init(tv, ti);

  float sq_own = 1.0f;   // this thread's query column scale
  if constexpr (I8) sq_own = sq_g[tid];
  const long long ld = d;   // row stride in bytes (1 B/elem)

  for (long long panel = blockIdx.x; panel < n_panels; panel += gridDim.x) {
    const long long prow = panel * F8_BM;

    unsigned int aw[F8_BM / 32];
    if constexpr (FILTERED) {
      unsigned int any = 0;
#pragma unroll
      for (int h = 0; h < F8_BM / 32; ++h) {
        aw[h] = allow[(prow >> 5) + h];
        any |= aw[h];
      }
      if (any == 0) continue;
    }

    acc_t acc[F8_MW][4];
#pragma unroll
    for (int m = 0; m < F8_MW; ++m)
#pragma unroll
      for (int nn = 0; nn < 4; ++nn) acc[m][nn] = acc_t{};

    for (int kt = 0; kt < d; kt += F8_BK) {
      // ---- stage A (96x128 B = 12 KB) and B (256x128 B = 32 KB): 1 KB
      // per global_load_lds chunk, global source pre-swizzled ----
#pragma unroll
      for (int it = 0; it < F8_BM / 32; ++it) {
        int chunk = wc * (F8_BM / 32) + it;
        int x = chunk * 1024 + lane * 16;
        int p = swz8(x);
        const G_AS unsigned int* gp = (const G_AS unsigned int*)(
            (const char*)db + (prow + (p >> 7)) * ld + (long long)kt +
            (p & 127));
        L_AS unsigned int* lp = (L_AS unsigned int*)(sA + chunk * 1024);
        __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
      }
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        int chunk = wc * 8 + it;
        int x = chunk * 1024 + lane * 16;
        int p = swz8(x);
        const G_AS unsigned int* gp = (const G_AS unsigned int*)(
            (const char*)qs + (long long)(p >> 7) * ld + (long long)kt +
            (p & 127));
        L_AS unsigned int* lp = (L_AS unsigned int*)(sB + chunk * 1024);
        __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
      }
      __syncthreads();

      // ---- MFMA: k-steps of KS over the staged 128 B rows; a fragment is
      // KS/4 bytes per lane (byte == elem offset), at most the 16 B slot
      // the row-XOR swizzle keeps whole ----
#pragma unroll
      for (int ks = 0; ks < F8_BK / KS; ++ks) {
        const int kb = ks * KS + (lane >> 4) * (KS / 4);
        frag_t bfr[4];
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
          int c = wc * 64 + nn * 16 + (lane & 15);
          bfr[nn] = *reinterpret_cast<const frag_t*>(sB + swz8(c * 128 + kb));
        }
#pragma unroll
        for (int m = 0; m < F8_MW; ++m) {
          int r = m * 16 + (lane & 15);
          frag_t af = *reinterpret_cast<const frag_t*>(sA + swz8(r * 128 + kb));
#pragma unroll
          for (int nn = 0; nn < 4; ++nn) {
            if constexpr (I8)
              acc[m][nn] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                  af, bfr[nn], acc[m][nn], 0, 0, 0);
            else
              acc[m][nn] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                  af, bfr[nn], acc[m][nn], 0, 0, 0);
          }
        }
      }
      __syncthreads();
    }

    // ---- epilogue: accumulators through the transposed LDS block, 32 rows
    // at a time; int8 dots are scaled to float on the way into the lists ----
#pragma unroll
    for (int h = 0; h < F8_BM / 32; ++h) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        int m = h * 2 + mi;
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) {
          int col = wc * 64 + nn * 16 + (lane & 15);
          int srow = mi * 16 + (lane >> 4) * 4;
          *reinterpret_cast<acc_t*>(sT + col * 36 + srow) = acc[m][nn];
        }
      }
      __syncthreads();
      const long long grow0 = prow + (long long)h * 32;
#pragma unroll
      for (int j = 0; j < 32; j += 4) {
        acc_t v = *reinterpret_cast<const acc_t*>(sT + tid * 36 + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long row = grow0 + j + e;
          float s = (float)v[e];
          if constexpr (I8) s = s * sa_g[row] * sq_own;
          bool ok = s > tv[F8_KCAND - 1];
          if constexpr (FILTERED) ok = ok && ((aw[h] >> (j + e)) & 1u);
          if (ok) topk_insert(tv, ti, s, (int)row);
        }
      }
      __syncthreads();
    }
  }

  long long slot = (long long)blockIdx.x * F8_BN + tid;
#pragma unroll
  for (int i = 0; i < F8_KCAND; ++i) {
    cand_score[slot * F8_KCAND + i] = tv[i];
    cand_idx[slot * F8_KCAND + i] = ti[i];
  }
}

// Checks shared by both formats, candidate allocation, launch and merge.
// db / q have passed the caller's dtype check; sa / sq are null for fp8.
template <int FMT>
static std::tuple<at::Tensor, at::Tensor> knn_q8(
    const char* who, const at::Tensor& db, const float* sa,
    const at::Tensor& q, const float* sq, long long row_base, int k_out,
    const c10::optional<at::Tensor>& allow) {
  long long n = db.size(0);
  int d = (int)db.size(1);
  TORCH_CHECK(q.size(0) == F8_BN, who, ": q must be padded to ", F8_BN);
  TORCH_CHECK(q.size(1) == d, "dim mismatch");
  TORCH_CHECK(d % F8_BK == 0, who, " needs D % 128 == 0");
  TORCH_CHECK(n % F8_BM == 0, who, " needs N % ", F8_BM, " == 0");
  TORCH_CHECK(n < (1LL << 31), "shard too large for int32 local rows");
  TORCH_CHECK(k_out >= 1 && k_out <= F8_KCAND);
  const unsigned int* allow_p = nullptr;
  if (allow.has_value()) allow_p = check_allow_mask(*allow, db, n, who);

  long long n_panels = n / F8_BM;
  int max_grid = 7680;
  if (const char* g = getenv("NORNICDB_KNN_GRID")) max_grid = atoi(g);
  int grid = (int)std::min<long long>(n_panels, max_grid);
  auto stream = at::hip::getCurrentHIPStream().stream();

  auto opts_f = db.options().dtype(at::kFloat);
  at::Tensor cand_s = at::empty({grid, F8_BN, F8_KCAND}, opts_f);
  at::Tensor cand_i = at::empty({grid, F8_BN, F8_KCAND},
                                db.options().dtype(at::kInt));

  auto launch = allow_p ? k_knn_q8<FMT, true> : k_knn_q8<FMT, false>;
  hipLaunchKernelGGL(launch, dim3(grid), dim3(F8_NTHREADS), 0, stream,
                     (const unsigned char*)db.data_ptr(), sa,
                     (const unsigned char*)q.data_ptr(), sq, n_panels, d,
                     row_base, cand_s.data_ptr<float>(),
                     cand_i.data_ptr<int>(), allow_p);
  HIP_CHECK_LAST();

  at::Tensor out_s = at::empty({F8_BN, k_out}, opts_f);
  at::Tensor out_i = at::empty({F8_BN, k_out},
                               db.options().dtype(at::kLong));
  topk_merge(cand_s, cand_i, grid, F8_BN, k_out, row_base, out_s, out_i,
             stream);
  return {out_s, out_i};
}

std::tuple<at::Tensor, at::Tensor> knn_i8(at::Tensor db, at::Tensor sa,
                                          at::Tensor q, at::Tensor sq,
                                          long long row_base, int k_out,
                                          c10::optional<at::Tensor> allow) {
  TORCH_CHECK(db.is_cuda() && db.dim() == 2 && db.is_contiguous() &&
                  db.scalar_type() == at::kChar,
              "knn_i8: db must be contiguous 2D int8 CUDA");
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.is_contiguous() &&
                  q.scalar_type() == at::kChar,
              "knn_i8: q must be contiguous 2D int8 CUDA");
  TORCH_CHECK(sa.scalar_type() == at::kFloat && sa.is_contiguous() &&
              sa.numel() == db.size(0), "knn_i8: sa must be fp32 [N]");
  TORCH_CHECK(sq.scalar_type() == at::kFloat && sq.is_contiguous() &&
              sq.numel() == F8_BN, "knn_i8: sq must be fp32 [256]");
  return knn_q8<Q8_FMT_I8>("knn_i8", db, sa.data_ptr<float>(), q,
                           sq.data_ptr<float>(), row_base, k_out, allow);
}

std::tuple<at::Tensor, at::Tensor> knn_fp8(at::Tensor db, at::Tensor q,
                                           long long row_base, int k_out,
                                           c10::optional<at::Tensor> allow) {
  TORCH_CHECK(db.is_cuda() && db.dim() == 2 && db.is_contiguous() &&
                  db.scalar_type() == at::kByte,
              "knn_fp8: db must be contiguous 2D uint8 (e4m3fn bits) CUDA");
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.is_contiguous() &&
                  q.scalar_type() == at::kByte,
              "knn_fp8: q must be contiguous 2D uint8 (e4m3fn bits) CUDA");
  return knn_q8<Q8_FMT_FP8>("knn_fp8", db, nullptr, q, nullptr, row_base,
                            k_out, allow);
}

// rows of one quantised panel (the kernel route consumes whole panels)
long long knn_q8_bm_value() { return F8_BM; }

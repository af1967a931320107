// Tier-1 vector kernels for NornicDB-AMD: L2 normalize, synthetic corpus
// generation, fused cosine-score + top-k (GEMV path for small query batches)
// and the IVF probe-list scan. Selection itself (register lists, cross-block
// merge) is topk.h.
//
// Re-designs (not ports of) the reference's CUDA kernels
// (reference: pkg/gpu/cuda/cuda_kernels.cu:185-460 — 1-thread-per-vector
// norms and a <<<1,1>>> top-k): here every kernel is wave64-shaped,
// vector-loaded (short8 = 8 x bf16 per lane) and fused so the embedding
// matrix is read exactly once per query batch.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"
#include "allow_mask.h"
#include "topk.h"

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
// in flight with the row's data, as sa[row] in k_ivf_scan_q8) and added
// once, in fp32, after the 16-lane butterfly has completed the dot product.
// Biases must be finite and far above the -1e30 list sentinel; the kernel
// does not test for that. BIASED=false never touches `row_bias`.
// ---------------------------------------------------------------------------
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));

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

// ---------------------------------------------------------------------------
// IVF probe-list scan: fused gather + cosine-score + per-block top-K.
//
// The corpus stays in slot order; an inverted list is a CSR slice of slot
// numbers (list_rows[list_off[c] .. list_off[c+1])). One 256-thread block
// serves one (query, probe, split) triple: it stages its query in LDS and
// its 16 lane-groups stride through the list's entries, each group scoring
// one gathered row per step with the gemv kernel's dot product (a row is
// d*2 contiguous bytes, so every 16-lane load is still fully coalesced).
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
//
// ivf_block(), ivf_list_range() and ivf_rank_merge() are the parts every
// scan kernel shares.
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
// means there is nothing to scan. Kernels call this behind their query
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

template <int K, bool FILTERED>
__global__ void __launch_bounds__(256)
k_ivf_scan_bf16(const unsigned short* __restrict__ db,
                const unsigned short* __restrict__ qs,
                const int* __restrict__ probes,
                const int* __restrict__ list_off,
                const int* __restrict__ list_rows,
                int n_lists, long long n_entries, int n_probe, int p_eff,
                int split, int tail_start, int n, int d, int q_count,
                long long row_base,
                float* __restrict__ cand_score,
                long long* __restrict__ cand_idx,
                const unsigned int* __restrict__ allow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  unsigned short* s_q = reinterpret_cast<unsigned short*>(s_raw);  // [d]
  float* s_ls = reinterpret_cast<float*>(s_raw + (size_t)d * 2);   // [16][K]
  int* s_li = reinterpret_cast<int*>(s_ls + 16 * K);               // [16][K]

  const int lane = threadIdx.x & (WAVE - 1);
  const int grp = lane >> 4;
  const int gl = lane & 15;
  const int wid = threadIdx.x / WAVE;
  const int g16 = wid * 4 + grp;    // lane-group within the block, 0..15

  const IvfBlock blk = ivf_block(p_eff, split);
  const int sp = blk.sp, p = blk.p, q = blk.q;

  for (int i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
    *reinterpret_cast<short8v*>(s_q + i) =
        *reinterpret_cast<const short8v*>(qs + (long long)q * d + i);
  }
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
      const unsigned short* rp = db + (long long)row * d + gl * 8;
      float acc = 0.0f;
#pragma unroll 8
      for (int jj = 0; jj < nj; ++jj) {
        short8v v = *reinterpret_cast<const short8v*>(rp + jj * 128);
        short8v qv = *reinterpret_cast<const short8v*>(s_q + jj * 128 + gl * 8);
        const bf16x2v* xa = reinterpret_cast<const bf16x2v*>(&v);
        const bf16x2v* qa = reinterpret_cast<const bf16x2v*>(&qv);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc = __builtin_amdgcn_fdot2_f32_bf16(xa[j], qa[j], acc, false);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        acc += __shfl_xor(acc, off, WAVE);
      // same score in all 16 lanes of the group: uniform insert
      if (acc > tv[K - 1]) topk_insert(tv, ti, acc, row);
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

// ---------------------------------------------------------------------------
// The same scan over a 1-byte-per-element corpus: symmetric int8 with
// per-row scales, or OCP e4m3 fp8. Block contract, list walk, insert and
// epilogue are those of k_ivf_scan_bf16; only the row score differs. The
// block decode (ivf_block, ivf_list_range), the insert (topk.h) and the epilogue
// (ivf_rank_merge) are shared as force-inlined helpers: compiled with them,
// every scan kernel keeps the registers, LDS and zero scratch it had with
// its own copy of the text (table in profiles/README.md, "Top-k core
// refactor"). The list walk is still written out in both kernels. A row is
// d contiguous bytes: per 128 elements each of a group's 16 lanes loads 8
// of them, against 8 query bytes from LDS.
//
// int8: the query arrives quantised (int8 [Q][d] and its scale sq[q]);
//   v_dot4 accumulates into an int32 that the butterfly reduces exactly,
//   score = float(dot) * sa[row] * sq[q] as in k_knn_q8. sa is indexed by
//   slot number and loaded ahead of the row's data.
// fp8: row and query bytes are converted in pairs (v_cvt_pk_f32_fp8, exact)
//   and accumulated in fp32.
// ---------------------------------------------------------------------------
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));   // 8B

template <int K, bool FILTERED, int FMT>
__global__ void __launch_bounds__(256)
k_ivf_scan_q8(const unsigned char* __restrict__ db,
              const unsigned char* __restrict__ qs,
              const float* __restrict__ sa,    // [n], int8 only
              const float* __restrict__ sq,    // [q_count], int8 only
              const int* __restrict__ probes,
              const int* __restrict__ list_off,
              const int* __restrict__ list_rows,
              int n_lists, long long n_entries, int n_probe, int p_eff,
              int split, int tail_start, int n, int d, int q_count,
              long long row_base,
              float* __restrict__ cand_score,
              long long* __restrict__ cand_idx,
              const unsigned int* __restrict__ allow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  unsigned char* s_q = s_raw;                                      // [d]
  float* s_ls = reinterpret_cast<float*>(s_raw + (size_t)d);       // [16][K]
  int* s_li = reinterpret_cast<int*>(s_ls + 16 * K);               // [16][K]

  const int lane = threadIdx.x & (WAVE - 1);
  const int grp = lane >> 4;
  const int gl = lane & 15;
  const int wid = threadIdx.x / WAVE;
  const int g16 = wid * 4 + grp;    // lane-group within the block, 0..15

  const IvfBlock blk = ivf_block(p_eff, split);
  const int sp = blk.sp, p = blk.p, q = blk.q;

  for (int i = threadIdx.x * 8; i < d; i += blockDim.x * 8) {
    *reinterpret_cast<uint2v*>(s_q + i) =
        *reinterpret_cast<const uint2v*>(qs + (long long)q * d + i);
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
      const unsigned char* rp = db + (long long)row * d + gl * 8;
      const unsigned char* qp = s_q + gl * 8;
      float score;
      if constexpr (FMT == Q8_FMT_I8) {
        // its own cache line per row: in flight with the row's data
        const float row_scale = sa[row];
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
        score = (float)acc * row_scale * q_scale;
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
        score = acc;
      }
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


// ---------------------------------------------------------------------------
// IVF scan + merge. probes [Q][P] int32 (any value outside [0, C) skips);
// list_off [C+1] / list_rows [M] int32 CSR of slot numbers below tail_start;
// rows [tail_start, N) are scanned by every query. max_len is the longest
// list, recorded when the lists were built (no device sync per search).
// ivf_scan (bf16), ivf_scan_i8 and ivf_scan_fp8 share the argument checks,
// the grid and the merge; they differ in the corpus / query dtype and in
// the scan kernel.
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

// Allocates the [W][Q][K] candidates, has `scan(blocks, lds_bytes, cand_s,
// cand_i)` launch the scan kernel over them (q_bytes of LDS hold the
// query) and merges them into [Q][k_out].
template <int K, typename Scan>
static std::tuple<at::Tensor, at::Tensor> ivf_scan_merge(
    const char* who, const IvfPlan& pl, const at::Tensor& db, size_t q_bytes,
    Scan scan) {
  auto opts_f = db.options().dtype(at::kFloat);
  auto opts_i = db.options().dtype(at::kLong);
  const long long w = (long long)pl.p_eff * pl.split;
  at::Tensor out_s = at::empty({pl.qc, pl.k_out}, opts_f);
  at::Tensor out_i = at::empty({pl.qc, pl.k_out}, opts_i);
  at::Tensor cand_s = at::empty({w, pl.qc, K}, opts_f);
  at::Tensor cand_i = at::empty({w, pl.qc, K}, opts_i);
  const size_t lds = q_bytes + (size_t)16 * K * 8;
  TORCH_CHECK(lds <= 64 * 1024, who, ": D too large for the LDS query tile");
  scan(dim3((unsigned)(w * pl.qc)), lds, cand_s.data_ptr<float>(),
       reinterpret_cast<long long*>(cand_i.data_ptr<int64_t>()));
  HIP_CHECK_LAST();
  // the scan added row_base to its ids
  topk_merge(cand_s, cand_i, w, pl.qc, pl.k_out, 0, out_s, out_i,
             cur_stream());
  return {out_s, out_i};
}

static std::tuple<at::Tensor, at::Tensor> ivf_nothing_to_scan(
    const IvfPlan& pl, const at::Tensor& db) {
  return {at::full({pl.qc, pl.k_out}, -1e30f, db.options().dtype(at::kFloat)),
          at::full({pl.qc, pl.k_out}, -1LL, db.options().dtype(at::kLong))};
}

template <int K>
static std::tuple<at::Tensor, at::Tensor> ivf_scan_bf16_run(
    const IvfPlan& pl, const at::Tensor& db, const at::Tensor& q,
    const at::Tensor& probes, const at::Tensor& list_off,
    const at::Tensor& list_rows) {
  auto kern = pl.allow_p ? k_ivf_scan_bf16<K, true> : k_ivf_scan_bf16<K, false>;
  return ivf_scan_merge<K>(
      "ivf_scan", pl, db, (size_t)pl.d * 2,
      [&](dim3 grid, size_t lds, float* cand_s, long long* cand_i) {
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, cur_stream(),
                           (const unsigned short*)db.data_ptr(),
                           (const unsigned short*)q.data_ptr(),
                           probes.data_ptr<int>(), list_off.data_ptr<int>(),
                           list_rows.data_ptr<int>(),
                           (int)list_off.numel() - 1,
                           (long long)list_rows.numel(), pl.n_probe, pl.p_eff,
                           pl.split, pl.tail_start, pl.n, pl.d, pl.qc,
                           pl.row_base, cand_s, cand_i, pl.allow_p);
      });
}

std::tuple<at::Tensor, at::Tensor> ivf_scan(
    at::Tensor db, at::Tensor q, at::Tensor probes, at::Tensor list_off,
    at::Tensor list_rows, long long tail_start, long long max_len,
    long long row_base, int k_out, c10::optional<at::Tensor> allow) {
  const IvfPlan pl = ivf_scan_plan("ivf_scan", db, at::kBFloat16, "bf16", q,
                                   at::kBFloat16, probes, list_off, list_rows,
                                   tail_start, max_len, row_base, k_out, allow);
  if (pl.p_eff == 0) return ivf_nothing_to_scan(pl, db);
  if (k_out <= 16)
    return ivf_scan_bf16_run<16>(pl, db, q, probes, list_off, list_rows);
  return ivf_scan_bf16_run<64>(pl, db, q, probes, list_off, list_rows);
}

// sa / sq are null for fp8
template <int K, int FMT>
static std::tuple<at::Tensor, at::Tensor> ivf_scan_q8_run(
    const char* who, const IvfPlan& pl, const at::Tensor& db,
    const at::Tensor& q, const float* sa, const float* sq,
    const at::Tensor& probes, const at::Tensor& list_off,
    const at::Tensor& list_rows) {
  auto kern = pl.allow_p ? k_ivf_scan_q8<K, true, FMT>
                         : k_ivf_scan_q8<K, false, FMT>;
  return ivf_scan_merge<K>(
      who, pl, db, (size_t)pl.d,
      [&](dim3 grid, size_t lds, float* cand_s, long long* cand_i) {
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, cur_stream(),
                           (const unsigned char*)db.data_ptr(),
                           (const unsigned char*)q.data_ptr(), sa, sq,
                           probes.data_ptr<int>(), list_off.data_ptr<int>(),
                           list_rows.data_ptr<int>(),
                           (int)list_off.numel() - 1,
                           (long long)list_rows.numel(), pl.n_probe, pl.p_eff,
                           pl.split, pl.tail_start, pl.n, pl.d, pl.qc,
                           pl.row_base, cand_s, cand_i, pl.allow_p);
      });
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
    return ivf_scan_q8_run<16, Q8_FMT_I8>(who, pl, db, q, sap, sqp, probes,
                                           list_off, list_rows);
  return ivf_scan_q8_run<64, Q8_FMT_I8>(who, pl, db, q, sap, sqp, probes,
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
    return ivf_scan_q8_run<16, Q8_FMT_FP8>(who, pl, db, q, nullptr, nullptr,
                                            probes, list_off, list_rows);
  return ivf_scan_q8_run<64, Q8_FMT_FP8>(who, pl, db, q, nullptr, nullptr,
                                          probes, list_off, list_rows);
}

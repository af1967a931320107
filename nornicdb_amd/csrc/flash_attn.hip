// Non-causal flash attention forward for the encoder: head_dim 64, bf16,
// no mask (padded batches fall back to torch sdpa in python).
//
// q,k,v: [B, S, H, 64] bf16 views (head stride 64, last dim contiguous,
// batch/seq strides free). out: contiguous [B, S, H, 64]. S % 64 == 0.
//
// Structure (k_flash_attn_nc):
//   - Workgroup = 8 waves = 256 query rows of one (batch, head); wave w owns
//     the 32 rows [32w, 32w+32). Grid (B*H, ceil(S/256)). At S <= 256 the K
//     and V of a head pass through the load path exactly once.
//   - K/V walked in 64-key tiles through a 2-deep LDS ring. The 512 threads
//     each carry one 16-byte piece of K and one of V per tile: the global
//     loads of tile t+1 are issued before tile t's compute and written to
//     the other ring slot after it, one barrier per tile.
//   - Swapped QK^T with mfma_f32_32x32x16_bf16: X = K_tile * Q^T, so a query
//     row's 64 scores sit in 32 registers of lane l and 32 of lane l^32. Row
//     max and row sum are in-register chains plus one permlane32_swap each.
//     No shuffles, no P buffer in LDS.
//   - P (bf16) is fed from the X registers as the B operand of
//     O^T = V^T * P^T. Element j of lane half h of k-step s is ROW
//     16s + 8(j>>2) + 4h + (j&3) of the 32-row X block, but the MFMA sums it
//     as k = 16s + 8h + j. So the K fragment puts key 16s + 8h + 4a + b in A
//     row 16s + 8a + 4h + b (bits 2 and 3 of the row swapped): PV then sums
//     the keys in natural order and V^T is fetched in natural order with
//     ds_read_b64_tr_b16 from the row-major V tile.
//   - Rounding steps are those of the 16x16x32 kernel this one replaced, so
//     that results stay what they were: scores summed over d in ascending
//     blocks of 8, p = exp2(fma(x, scale, -m) * log2e), the row sum as
//     ((p[j] + p[16+j]) + p[32+j]) + p[48+j] for j = 0..15 followed by a
//     pairwise tree over j, l = fma(l, alpha, sum), PV summed over keys in
//     ascending blocks of 8, and a correctly rounded acc / l.
//   - K tile: 128-byte rows, 16-byte chunk c of row r at chunk c ^ ((r>>1)&7):
//     the ds_read_b128 row reads (16-lane groups, same chunk, rows distinct)
//     hit 16 distinct 16-byte slots. V tile: chunk c ^ (4*((r>>1)&1)): the
//     four rows of one transposed read (32 lanes = 4 rows x 64 bytes) land on
//     256 distinct bytes of the bank row.
//   - Online softmax keeps the exact per-tile max; l and O accumulate in
//     fp32; P is rounded to bf16 (RNE) before PV.
//   - Epilogue: O^T has the query on the lane; lanes l and l+32 exchange
//     halves with permlane32_swap so each lane stores 16-byte pieces.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef __bf16 fa_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 fa_bf16x4 __attribute__((ext_vector_type(4)));
typedef short fa_short4 __attribute__((ext_vector_type(4)));
typedef float fa_f32x16 __attribute__((ext_vector_type(16)));

#define FA_D 64            // head dim
#define FA_KT 64           // keys per tile
#define FA_QW 32           // query rows per wave
#define FA_WAVES 8
#define FA_QB (FA_QW * FA_WAVES)   // 256 query rows per workgroup
#define FA_TILE_BYTES (FA_KT * FA_D * 2)   // 8 KB
#define FA_L_AS __attribute__((address_space(3)))

// Byte offset of 16-byte chunk c (0..7) of row r inside a K / V tile.
DEV_INLINE int fa_k_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }
DEV_INLINE int fa_v_off(int r, int c) { return r * 128 + ((c ^ (((r >> 1) & 1) << 2)) << 4); }

// 4 rows x 16 columns of bf16 read transposed: lane i of a 16-lane group gets
// column i of the four rows whose addresses the group's lanes supply.
DEV_INLINE fa_short4 fa_read_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((FA_L_AS fa_short4*)p);
}

DEV_INLINE unsigned int fa_pack2(float lo, float hi) {
  typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
  bf2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned int, v);
}

__global__ __launch_bounds__(FA_WAVES * WAVE) void k_flash_attn_nc(
    const unsigned short* __restrict__ Q, const unsigned short* __restrict__ K,
    const unsigned short* __restrict__ V, unsigned short* __restrict__ O,
    int n_heads, int s, float scale,
    long long q_bs, long long q_ss,   // batch/seq strides (elements)
    long long k_bs, long long k_ss,
    long long v_bs, long long v_ss) {
  // ring slot i: K tile at 2*i*8K, V tile at (2*i+1)*8K
  __shared__ __attribute__((aligned(16))) char smem[4 * FA_TILE_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int b = blockIdx.x / n_heads;
  const int h = blockIdx.x % n_heads;
  const long long hoff = (long long)h * FA_D;
  const int lr = lane & 31;     // query row of this lane inside the wave
  const int lh = lane >> 5;     // lane half

  // Query row of this lane. Waves past S (S not a multiple of 256) keep
  // staging and taking barriers on a clamped row and skip the store.
  const int qrow = blockIdx.y * FA_QB + wid * FA_QW + lr;
  const bool active = blockIdx.y * FA_QB + wid * FA_QW < s;   // wave-uniform
  const int qrow_c = min(qrow, s - 1);

  // ---- Q fragments (B operand of X = K * Q^T), held for the whole kernel:
  // lane holds Q[qrow][16*ks + 8*lh + j], ks = 0..3
  fa_bf16x8 qf[4];
  {
    const unsigned short* qp = Q + b * q_bs + (long long)qrow_c * q_ss + hoff;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      qf[ks] = (fa_bf16x8)(*reinterpret_cast<const short8v*>(qp + ks * 16 + lh * 8));
  }

  // ---- staging: thread tid carries chunk (tid&7) of row (tid>>3) ----
  const int st_r = tid >> 3, st_c = tid & 7;
  const unsigned short* kp = K + b * k_bs + (long long)st_r * k_ss + hoff + st_c * 8;
  const unsigned short* vp = V + b * v_bs + (long long)st_r * v_ss + hoff + st_c * 8;
  const int st_koff = fa_k_off(st_r, st_c);
  const int st_voff = FA_TILE_BYTES + fa_v_off(st_r, st_c);

  // ---- read addresses inside a ring slot ----
  // K row read for key block kb, k-step ks: A row lr holds key
  // 32*kb + krow (lr with bits 2 and 3 swapped), chunk 2*ks + lh. The swap
  // maps each 16-lane read group onto itself, so the reads stay conflict-free.
  // (32*kb keeps (r>>1)&7, so kb is a +4096 byte immediate.)
  const int krow = (lr & 19) | ((lr & 4) << 1) | ((lr & 8) >> 1);
  int k_rd[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) k_rd[ks] = fa_k_off(krow, 2 * ks + lh);
  // V transposed read for d block db, first key r0 (multiple of 16) + 8*lh
  // (+4 for the second read): 16-lane group g covers columns
  // 32*db + 16*(g&1) .. +15; lane 4q+p of the group supplies row r0 + q,
  // columns 4p .. 4p+3. The first row is a multiple of 4, so
  // (row>>1)&1 == q>>1 for every tile row the lane reads.
  const int vq = (lane >> 2) & 3, vpp = lane & 3, vg1 = (lane >> 4) & 1;
  int v_rd[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
    v_rd[db] = FA_TILE_BYTES + fa_v_off(8 * lh + vq, 4 * db + 2 * vg1 + (vpp >> 1)) +
               8 * (vpp & 1);

  const float log2e = 1.44269504f;
  float m_run = -1e30f;   // running max of score * scale
  float l_run = 0.f;      // row sum (the same in lanes l and l+32)
  fa_f32x16 acc[2];       // O^T: acc[db][r] = O[qrow][32db + (r&3)+8(r>>2)+4lh]
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[db][r] = 0.f;

  const int nt = s / FA_KT;

  // prologue: tile 0 into ring slot 0
  {
    short8v kr = *reinterpret_cast<const short8v*>(kp);
    short8v vr = *reinterpret_cast<const short8v*>(vp);
    *reinterpret_cast<short8v*>(smem + st_koff) = kr;
    *reinterpret_cast<short8v*>(smem + st_voff) = vr;
  }
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    const char* slot = smem + (t & 1) * (2 * FA_TILE_BYTES);
    const bool more = t + 1 < nt;   // block-uniform
    short8v kr, vr;
    if (more) {
      kr = *reinterpret_cast<const short8v*>(kp + (long long)(t + 1) * FA_KT * k_ss);
      vr = *reinterpret_cast<const short8v*>(vp + (long long)(t + 1) * FA_KT * v_ss);
    }

    // ---- X = K_tile * Q^T:
    // x[kb][r] = score(key 32kb + 16(r>>3) + 8lh + 4((r>>2)&1) + (r&3), qrow)
    fa_f32x16 x[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      fa_f32x16 c;
#pragma unroll
      for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        fa_bf16x8 kf = (fa_bf16x8)(*reinterpret_cast<const short8v*>(
            slot + k_rd[ks] + kb * 4096));
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], c, 0, 0, 0);
      }
      x[kb] = c;
    }

    // ---- online softmax, exact per-tile max ----
    float mx = x[0][0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, x[0][r]);
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, x[1][r]);
    {
      unsigned int u = __builtin_bit_cast(unsigned int, mx);
      auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
      mx = fmaxf(__builtin_bit_cast(float, (unsigned int)sw[0]),
                 __builtin_bit_cast(float, (unsigned int)sw[1]));
    }
    const float m_new = fmaxf(m_run, mx * scale);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * log2e);
    m_run = m_new;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        x[kb][r] = __builtin_amdgcn_exp2f(
            __builtin_fmaf(x[kb][r], scale, -m_new) * log2e);
    // row sum: column j = 8lh + 4a + b of the tile's four 16-key groups
    // first, then the pairwise tree over j (j^1, j^2, j^4 in this lane,
    // j^8 in lane l^32)
    float t2[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      float c[4];
#pragma unroll
      for (int bq = 0; bq < 4; ++bq)
        c[bq] = ((x[0][4 * a + bq] + x[0][8 + 4 * a + bq]) + x[1][4 * a + bq]) +
                x[1][8 + 4 * a + bq];
      t2[a] = (c[0] + c[1]) + (c[2] + c[3]);
    }
    float lsum = t2[0] + t2[1];
    {
      unsigned int u = __builtin_bit_cast(unsigned int, lsum);
      auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
      lsum = __builtin_bit_cast(float, (unsigned int)sw[0]) +
             __builtin_bit_cast(float, (unsigned int)sw[1]);
    }
    l_run = __builtin_fmaf(l_run, alpha, lsum);
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[db][r] *= alpha;

    // ---- O^T += V^T * P^T ----
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        // B operand: registers 8st..8st+7 of x[kb], packed to bf16
        uint4v pw;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          pw[j] = fa_pack2(x[kb][8 * st + 2 * j], x[kb][8 * st + 2 * j + 1]);
        fa_bf16x8 pf = __builtin_bit_cast(fa_bf16x8, pw);
        // A operand: V[key 32kb + 16st + 8lh + j][32db + lr]
        const int r0 = (32 * kb + 16 * st) * 128;
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          fa_short4 lo = fa_read_tr(slot + v_rd[db] + r0);
          fa_short4 hi = fa_read_tr(slot + v_rd[db] + r0 + 4 * 128);
          short8v vf8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              (fa_bf16x8)vf8, pf, acc[db], 0, 0, 0);
        }
      }
    }

    if (more) {
      char* nslot = smem + ((t + 1) & 1) * (2 * FA_TILE_BYTES);
      *reinterpret_cast<short8v*>(nslot + st_koff) = kr;
      *reinterpret_cast<short8v*>(nslot + st_voff) = vr;
    }
    __syncthreads();
  }

  // ---- epilogue: normalise, store ----
  // acc / l correctly rounded without a division per element: with
  // inv_l = RN(1/l), q = RN(a*inv_l), e = a - q*l (exact in the fma),
  // RN(q + e*inv_l) is the correctly rounded quotient (Markstein).
  if (!active) return;
  const float l_fin = fmaxf(l_run, 1e-20f);
  const float inv_l = 1.0f / l_fin;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float a = acc[db][r];
      const float q = a * inv_l;
      acc[db][r] = __builtin_fmaf(__builtin_fmaf(-q, l_fin, a), inv_l, q);
    }
  unsigned short* op =
      O + ((long long)b * s + qrow) * ((long long)n_heads * FA_D) + hoff + lh * 8;
#pragma unroll
  for (int db = 0; db < 2; ++db) {
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      // column group k = 4db + g: this lane holds d = 8k + 4lh .. +3
      unsigned int ax = fa_pack2(acc[db][4 * g + 0], acc[db][4 * g + 1]);
      unsigned int ay = fa_pack2(acc[db][4 * g + 2], acc[db][4 * g + 3]);
      unsigned int bx = fa_pack2(acc[db][4 * g + 4], acc[db][4 * g + 5]);
      unsigned int by = fa_pack2(acc[db][4 * g + 6], acc[db][4 * g + 7]);
      auto sx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
      auto sy = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
      uint4v o4 = {(unsigned int)sx[0], (unsigned int)sy[0],
                   (unsigned int)sx[1], (unsigned int)sy[1]};
      // lanes 0-31: d = 8k .. 8k+7; lanes 32-63: d = 8k+8 .. 8k+15
      *reinterpret_cast<uint4v*>(op + 8 * (4 * db + g)) = o4;
    }
  }
}

at::Tensor flash_attn_nc(at::Tensor q, at::Tensor k, at::Tensor v) {
  // q,k,v: [B, S, H, 64] bf16 VIEWS — head stride must be 64 and the last
  // dim contiguous; batch/seq strides are free (so qkv.unbind(2) feeds in
  // without any transpose/copy). Returns contiguous [B, S, H, 64].
  TORCH_CHECK(q.is_cuda() && q.dim() == 4 && q.scalar_type() == at::kBFloat16,
              "flash_attn_nc: q [B,S,H,D] bf16");
  int B = (int)q.size(0), S = (int)q.size(1), H = (int)q.size(2),
      D = (int)q.size(3);
  TORCH_CHECK(D == 64, "flash_attn_nc supports head_dim 64");
  TORCH_CHECK(S > 0 && S % 64 == 0, "flash_attn_nc needs S % 64 == 0");
  for (auto* t : {&q, &k, &v}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kBFloat16 &&
                    t->sizes() == q.sizes(),
                "flash_attn_nc: q, k, v must be bf16 with one shape");
    TORCH_CHECK(t->stride(3) == 1 && t->stride(2) == D,
                "flash_attn_nc: head stride must be D, last dim contiguous");
    TORCH_CHECK(t->stride(0) % 8 == 0 && t->stride(1) % 8 == 0 &&
                    (reinterpret_cast<uintptr_t>(t->data_ptr()) & 15) == 0,
                "flash_attn_nc: rows must be 16-byte aligned");
  }
  at::Tensor o = at::empty({B, S, H, D}, q.options());
  if (B == 0 || H == 0) return o;
  float scale = 1.0f / sqrtf((float)D);
  dim3 grid(B * H, (S + FA_QB - 1) / FA_QB);
  hipLaunchKernelGGL(k_flash_attn_nc, grid, dim3(FA_WAVES * WAVE), 0,
                     at::hip::getCurrentHIPStream().stream(),
                     (const unsigned short*)q.data_ptr(),
                     (const unsigned short*)k.data_ptr(),
                     (const unsigned short*)v.data_ptr(),
                     (unsigned short*)o.data_ptr(), H, S, scale,
                     q.stride(0), q.stride(1), k.stride(0), k.stride(1),
                     v.stride(0), v.stride(1));
  HIP_CHECK_LAST();
  return o;
}

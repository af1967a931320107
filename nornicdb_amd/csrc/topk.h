// Top-k selection core shared by the kNN and IVF kernels.
//
// Device side: a thread keeps a descending K-list in registers (scores tv,
// ids ti; empty slots are (-1e30, -1)) and pushes candidates into it with a
// statically unrolled insertion chain. The comparison is a strict `>`, so of
// two equal scores the one inserted first stays ahead. Callers guard the
// insert themselves (`score > tv[K - 1]`, combined with their mask bit), so
// that the guard stays where their epilogue wants it.
//
// Host side: topk_merge() reduces the kernels' per-block candidate lists to
// the final [Q][k_out]. Its kernel lives in topk_merge.hip alone; a host
// function rather than a kernel template in this header, so that no kernel
// symbol is instantiated in two code objects.
#pragma once

#include "common.h"

template <int K, typename IDX>
DEV_INLINE void topk_init(float (&tv)[K], IDX (&ti)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) { tv[i] = -1e30f; ti[i] = -1; }
}

template <int K, typename IDX>
DEV_INLINE void topk_insert(float (&tv)[K], IDX (&ti)[K], float cs, IDX ci) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    bool ins = cs > tv[i];
    float ts = tv[i]; IDX tj = ti[i];
    tv[i] = ins ? cs : tv[i];
    ti[i] = ins ? ci : ti[i];
    cs = ins ? ts : cs; ci = ins ? tj : ci;
  }
}

// Order-preserving map of a float onto unsigned ints, for packed argmax.
DEV_INLINE unsigned int f32_mono(float f) {
  unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Merge candidate lists cand_s / cand_i [w][q_stride][K] into out_s / out_i
// [Q][k_out] (fp32, int64), one block per row of out_*, Q <= q_stride. K is
// cand_s's last dimension, one of 10, 16 or 64; cand_i is int32 or int64.
// An id < 0 marks an empty slot and comes out as -1, every other id as
// row_base + id (pass 0 when the candidates already hold global ids).
void topk_merge(const at::Tensor& cand_s, const at::Tensor& cand_i,
                long long w, int q_stride, int k_out, long long row_base,
                at::Tensor& out_s, at::Tensor& out_i, hipStream_t stream);

// BM25 posting-list scan for NornicDB-AMD: fused posting gather + score +
// per-block top-K over device-resident CSR postings, and its host code.
// The cross-block merge is topk.h's topk_merge().

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <algorithm>
#include <cstdlib>
#include "common.h"
#include "allow_mask.h"
#include "topk.h"

// ---------------------------------------------------------------------------
// Postings are a CSR over term ids: post_doc[post_off[t] .. post_off[t+1])
// are the slot numbers of the documents that hold term t, strictly
// ascending, post_tf their term frequencies; doc_len[slot] is a document's
// length. A query is T (term id, weight) columns; a posting contributes
//   w * tf / (tf + c0 + c1 * doc_len[slot])
// to its document, and a document's score is the sum over the columns in
// column order.
//
// Scoring is partitioned by document range, not by posting list: the slot
// space is cut into ranges of BM25_RANGE documents whose fp32 accumulators
// fit in 32 KB of LDS. Block (q, b) of a query's `bpq` blocks walks ranges
// b, b + bpq, ... For each range it finds the part of every term's slice
// that falls in the range (a wave-wide k-ary search, 64 probes per step;
// the block's 4 waves share out the terms) and then, term column by term
// column in order, adds that part's contributions into the accumulators.
// Inside one term every document appears once, so the adds are plain LDS
// read-modify-writes, and a barrier separates the terms: the sums are taken
// in a fixed order and no float atomic is used anywhere.
//
// Selection: the block keeps its K best in LDS, items [0, K). The threads
// read the accumulators back in chunks of at most BM25_CHUNK and append the
// ones that are touched (> 0), beat the K-th best and, when FILTERED, have
// their allow bit set, to items [K, K + cnt) through an LDS counter (an
// integer atomic; it orders nothing that is kept). Every item
// then finds its rank in the union by counting under the total order
// (score descending, slot ascending), and ranks < K form the new list. The
// order is total, so the result does not depend on the append order. A
// block visits slots in ascending order, so a later document that ties the
// K-th best loses to it: the strict `>` against the threshold is that rule.
//
// A block ends with ONE candidate list of K in topk_merge()'s [W][Q][K]
// layout, W = bpq.
// ---------------------------------------------------------------------------

constexpr int BM25_RANGE = 8192;   // documents per range: 32 KB of fp32
constexpr int BM25_CHUNK = 1024;   // accumulators selected from per pass
constexpr int BM25_THREADS = 256;
constexpr int BM25_TGROUP = 32;    // term columns searched ahead of their adds

long long bm25_range_value() { return BM25_RANGE; }

// The part [e0, e1) of the ascending slice post_doc[s0, s1) whose slots lie
// in [lo_slot, hi_slot): two lower bounds, searched in lockstep so that
// their loads are in flight together. All 64 lanes of a wave call this with
// the same arguments and get the same answer. Every step probes 64 evenly
// spaced entries and keeps the one gap the answer lies in, so a 16M-entry
// slice takes 4 dependent loads.
DEV_INLINE void bm25_slice_bounds(const int* __restrict__ post_doc,
                                  long long s0, long long s1, int lo_slot,
                                  int hi_slot, int lane, long long& e0,
                                  long long& e1) {
  long long lo[2] = {s0, s0}, hi[2] = {s1, s1};
  const int target[2] = {lo_slot, hi_slot};
  while (hi[0] > lo[0] || hi[1] > lo[1]) {
    long long step[2];
    bool below[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      step[i] = (hi[i] - lo[i] + 63) / 64;
      const long long p = lo[i] + (long long)(lane + 1) * step[i] - 1;
      below[i] = hi[i] > lo[i] && p < hi[i] && post_doc[p] < target[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = __popcll(__ballot(below[i]));
      // entry lo + c*step - 1 is below the target; entry lo + (c+1)*step
      // - 1, if there is one, is not. A finished search (hi == lo) has
      // step 0 and stays where it is.
      const long long nlo = lo[i] + (long long)c * step[i];
      hi[i] = std::max(std::min(nlo + step[i] - 1, hi[i]), nlo);
      lo[i] = nlo;
    }
  }
  e0 = lo[0];
  e1 = lo[1];
}

template <int K, bool FILTERED>
__global__ void __launch_bounds__(BM25_THREADS)
k_bm25_scan(const long long* __restrict__ post_off,
            const int* __restrict__ post_doc,
            const int* __restrict__ post_tf,
            const int* __restrict__ doc_len,
            const int* __restrict__ q_terms,
            const float* __restrict__ q_w,
            float c0, float c1, int n_terms, long long n_post, int n,
            int t_count, int q_count, int bpq, int n_ranges,
            float* __restrict__ cand_score,
            long long* __restrict__ cand_idx,
            const unsigned int* __restrict__ allow) {
  __shared__ __attribute__((aligned(16))) float s_acc[BM25_RANGE];
  __shared__ float s_is[K + BM25_CHUNK];   // items: best K, then survivors
  __shared__ int s_ii[K + BM25_CHUNK];
  __shared__ float s_ns[K];                // the next best K
  __shared__ int s_ni[K];
  __shared__ int s_cnt;
  __shared__ long long s_e0[BM25_TGROUP];  // a term's postings in the range
  __shared__ long long s_e1[BM25_TGROUP];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int q = blockIdx.x / bpq;
  const int b = blockIdx.x % bpq;
  const int* qt = q_terms + (long long)q * t_count;
  const float* qw = q_w + (long long)q * t_count;

  for (int i = tid; i < BM25_RANGE; i += BM25_THREADS) s_acc[i] = 0.0f;
  for (int i = tid; i < K; i += BM25_THREADS) {
    s_is[i] = -1e30f;
    s_ii[i] = -1;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();

  int seen = 0;   // documents this block has selected from so far
  for (int r = b; r < n_ranges; r += bpq) {
    const int lo = r * BM25_RANGE;
    const int hi = (int)std::min<long long>((long long)lo + BM25_RANGE, n);
    const unsigned int span = (unsigned int)(hi - lo);

    // ---- accumulate, term by term ----
    bool any = false;
    for (int t0 = 0; t0 < t_count; t0 += BM25_TGROUP) {
      const int t1 = std::min(t0 + BM25_TGROUP, t_count);
      // the waves share out the group's searches, so that their dependent
      // loads run side by side instead of in front of every term
      __syncthreads();   // the bounds found before this are used up
      for (int t = t0 + wid; t < t1; t += BM25_THREADS / WAVE) {
        const int term = qt[t];
        long long e0 = 0, e1 = 0;
        if (term >= 0 && term < n_terms) {   // wave-uniform
          const long long s0 = std::max(post_off[term], 0LL);
          const long long s1 = std::min(post_off[term + 1], n_post);
          bm25_slice_bounds(post_doc, s0, s1, lo, hi, lane, e0, e1);
        }
        if (lane == 0) {
          s_e0[t - t0] = e0;
          s_e1[t - t0] = e1;
        }
      }
      __syncthreads();
      for (int t = t0; t < t1; ++t) {
        const long long e0 = s_e0[t - t0], e1 = s_e1[t - t0];
        if (e1 <= e0) continue;   // block-uniform
        any = true;
        const float w = qw[t];
#pragma unroll 4
        for (long long e = e0 + tid; e < e1; e += BM25_THREADS) {
          const unsigned int off =
              (unsigned int)post_doc[e] - (unsigned int)lo;
          if (off < span) {   // holds for ascending postings; keeps LDS and
                              // doc_len in bounds for any others
            const float tf = (float)post_tf[e];
            const float dl = (float)doc_len[lo + (int)off];
            s_acc[off] += w * tf / (tf + c0 + c1 * dl);
          }
        }
        __syncthreads();   // the next term may touch the same documents
      }
    }
    if (!any) continue;   // nothing touched: the accumulators are still 0

    // ---- select, and clear the accumulators for the next range ----
    for (int c = 0, size; c < BM25_RANGE && lo + c < hi; c += size) {
      // Ranking costs (K + survivors)^2. While the block has seen few
      // documents its threshold is low and most touched documents survive,
      // so the first chunks are short: 256, 256, 512, then BM25_CHUNK, each
      // as long as everything before it and aligned to its own size.
      size = seen < 512 ? 256 : seen < 1024 ? 512 : BM25_CHUNK;
      size = std::min(size, BM25_RANGE - c);
      seen += size;
      const float thr = s_is[K - 1];
      for (int j = 0; j < size; j += BM25_THREADS) {
        const int off = c + j + tid;
        const float a = s_acc[off];
        s_acc[off] = 0.0f;
        bool ok = a > 0.0f && a > thr;
        if constexpr (FILTERED) {
          if (ok) {
            const int slot = lo + off;
            ok = (allow[slot >> 5] >> (slot & 31)) & 1u;
          }
        }
        if (ok) {
          const int pos = K + atomicAdd(&s_cnt, 1);
          s_is[pos] = a;
          s_ii[pos] = lo + off;
        }
      }
      __syncthreads();
      const int cnt = s_cnt;
      if (cnt > 0) {   // block-uniform
        const int total = K + cnt;
        for (int x = tid; x < total; x += BM25_THREADS) {
          const float xs = s_is[x];
          const int xi = s_ii[x];
          int rank = 0;
          for (int y = 0; y < total; ++y) {
            const float ys = s_is[y];
            const int yi = s_ii[y];
            // slots are distinct except among the empty (-1e30, -1) items,
            // which their position orders
            rank += (ys > xs || (ys == xs && (yi < xi || (yi == xi && y < x))))
                        ? 1 : 0;
          }
          if (rank < K) {
            s_ns[rank] = xs;
            s_ni[rank] = xi;
          }
        }
        __syncthreads();
        for (int i = tid; i < K; i += BM25_THREADS) {
          s_is[i] = s_ns[i];
          s_ii[i] = s_ni[i];
        }
        if (tid == 0) s_cnt = 0;
      }
      __syncthreads();
    }
  }

  const long long out_base = ((long long)b * q_count + q) * K;
  for (int i = tid; i < K; i += BM25_THREADS) {
    cand_score[out_base + i] = s_is[i];
    cand_idx[out_base + i] = (long long)s_ii[i];
  }
}

// ===========================================================================
// Host wrapper
// ===========================================================================

template <int K>
static void bm25_scan_run(const at::Tensor& post_off, const at::Tensor& post_doc,
                          const at::Tensor& post_tf, const at::Tensor& doc_len,
                          const at::Tensor& q_terms, const at::Tensor& q_w,
                          float c0, float c1, int bpq, int n_ranges, int k_out,
                          const unsigned int* allow_p, at::Tensor& out_s,
                          at::Tensor& out_i) {
  const int qc = (int)q_terms.size(0);
  hipStream_t stream = at::hip::getCurrentHIPStream().stream();
  at::Tensor cand_s =
      at::empty({bpq, qc, K}, doc_len.options().dtype(at::kFloat));
  at::Tensor cand_i =
      at::empty({bpq, qc, K}, doc_len.options().dtype(at::kLong));
  auto kern = allow_p ? k_bm25_scan<K, true> : k_bm25_scan<K, false>;
  hipLaunchKernelGGL(
      kern, dim3((unsigned)((long long)qc * bpq)), dim3(BM25_THREADS), 0,
      stream,
      reinterpret_cast<const long long*>(post_off.data_ptr<int64_t>()),
      post_doc.data_ptr<int>(), post_tf.data_ptr<int>(),
      doc_len.data_ptr<int>(), q_terms.data_ptr<int>(),
      q_w.data_ptr<float>(), c0, c1, (int)post_off.numel() - 1,
      (long long)post_doc.numel(), (int)doc_len.numel(),
      (int)q_terms.size(1), qc, bpq, n_ranges, cand_s.data_ptr<float>(),
      reinterpret_cast<long long*>(cand_i.data_ptr<int64_t>()), allow_p);
  HIP_CHECK_LAST();
  topk_merge(cand_s, cand_i, bpq, qc, k_out, 0, out_s, out_i, stream);
}

// post_off [V+1] int64, post_doc / post_tf [M] int32, doc_len [n] int32;
// q_terms [Q][T] int32 (any id outside [0, V) skips), q_w [Q][T] fp32.
// Returns (scores [Q][k_out] fp32, slots [Q][k_out] int64), descending;
// unfilled slots are (-1e30, -1). Only documents with a score > 0 are
// returned.
std::tuple<at::Tensor, at::Tensor> bm25_scan(
    at::Tensor post_off, at::Tensor post_doc, at::Tensor post_tf,
    at::Tensor doc_len, at::Tensor q_terms, at::Tensor q_w, double c0,
    double c1, int k_out, c10::optional<at::Tensor> allow) {
  const char* who = "bm25_scan";
  TORCH_CHECK(post_off.is_cuda() && post_off.is_contiguous() &&
                  post_off.scalar_type() == at::kLong && post_off.dim() == 1 &&
                  post_off.numel() >= 1,
              who, ": post_off must be a contiguous int64 [V+1] CUDA tensor");
  for (const at::Tensor* t : {&post_doc, &post_tf, &doc_len})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == at::kInt && t->dim() == 1,
                who, ": post_doc, post_tf and doc_len must be contiguous 1D "
                "int32 CUDA tensors");
  TORCH_CHECK(q_terms.is_cuda() && q_terms.is_contiguous() &&
                  q_terms.scalar_type() == at::kInt && q_terms.dim() == 2,
              who, ": q_terms must be a contiguous int32 [Q, T] CUDA tensor");
  TORCH_CHECK(q_w.is_cuda() && q_w.is_contiguous() &&
                  q_w.scalar_type() == at::kFloat,
              who, ": q_w must be a contiguous fp32 CUDA tensor");
  TORCH_CHECK(q_w.sizes() == q_terms.sizes(), who,
              ": q_w must be shaped like q_terms");
  for (const at::Tensor* t : {&post_doc, &post_tf, &doc_len, &q_terms, &q_w})
    TORCH_CHECK(t->device() == post_off.device(), who,
                ": all tensors must be on post_off's device");
  TORCH_CHECK(post_tf.numel() == post_doc.numel(), who,
              ": post_tf must hold one entry per posting, M");
  const long long n = doc_len.numel();
  const long long qc = q_terms.size(0);
  const long long tc = q_terms.size(1);
  TORCH_CHECK(n <= 0x7fffffffLL, who, ": int32 slot numbers, n < 2^31");
  TORCH_CHECK(post_off.numel() - 1 <= 0x7fffffffLL, who,
              ": int32 term ids, V < 2^31");
  TORCH_CHECK(qc >= 1, who, ": need at least one query");
  TORCH_CHECK(k_out >= 1 && k_out <= 64, who, ": k_out must be in 1..64");
  const unsigned int* allow_p = nullptr;
  if (allow.has_value()) allow_p = check_allow_mask(*allow, doc_len, n, who);

  if (tc == 0 || post_doc.numel() == 0 || n == 0)
    return {at::full({qc, k_out}, -1e30f, doc_len.options().dtype(at::kFloat)),
            at::full({qc, k_out}, -1LL, doc_len.options().dtype(at::kLong))};

  // ~1024 blocks per call, as the IVF scan sizes its grid; a block that
  // owns several ranges walks them in turn
  long long cap = 1024;
  if (const char* g = getenv("NORNICDB_BM25_BLOCKS"))
    cap = std::max(atoll(g), 1LL);
  const long long n_ranges = (n + BM25_RANGE - 1) / BM25_RANGE;
  const long long bpq =
      std::min(n_ranges, std::max<long long>(cap / qc, 1));
  TORCH_CHECK(qc * bpq <= 0x7fffffffLL, who, ": grid too large");

  at::Tensor out_s = at::empty({qc, k_out}, doc_len.options().dtype(at::kFloat));
  at::Tensor out_i = at::empty({qc, k_out}, doc_len.options().dtype(at::kLong));
  if (k_out <= 16)
    bm25_scan_run<16>(post_off, post_doc, post_tf, doc_len, q_terms, q_w,
                      (float)c0, (float)c1, (int)bpq, (int)n_ranges, k_out,
                      allow_p, out_s, out_i);
  else
    bm25_scan_run<64>(post_off, post_doc, post_tf, doc_len, q_terms, q_w,
                      (float)c0, (float)c1, (int)bpq, (int)n_ranges, k_out,
                      allow_p, out_s, out_i);
  return {out_s, out_i};
}

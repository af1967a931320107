// Centrality kernels over CSR adjacency: multi-source BFS for closeness and
// the Brandes forward / backward sweeps for betweenness.
//
// Replaces the per-source CPU loops behind the reference's
// apoc.algo.closenessCentrality / apoc.algo.betweennessCentrality
// (reference apoc/algo/algo.go) for large graphs; the python loops in
// graph/algos.py stay as the small-graph path.
//
// CSR as in graph.hip: row_ptr [n+1] int64, col_idx [m] int32. Single device,
// whole graph per launch. Every kernel is a level-synchronous pull sweep in
// the row shape of k_pagerank_gather_thr: a wave claims 64 consecutive rows,
// a row of at most 64 edges is scanned serially by its lane, and longer rows
// (hubs) are redone by the whole wave, chosen by a ballot, with a fixed-tree
// wave reduction. A thread writes only the state of its own vertex, kernels
// talk to each other only across launch boundaries, and there are no float
// atomics: every result is bit-reproducible.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "common.h"

typedef unsigned long long u64;

// Edges per lane whose gathers the whole-wave pass over a hub row keeps in
// flight together. A hub row is one wave's work, so its time is the row's
// length / (64 * HUB_ILP) dependent memory round trips.
#define HUB_ILP 8

DEV_INLINE double wave_reduce_sum_f64(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

DEV_INLINE u64 wave_reduce_or(u64 x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off, WAVE);
  return x;
}

// ---------------------------------------------------------------------------
// Multi-source BFS level, 64 sources per machine word. Bit b of frontier /
// visited / next belongs to source b of the batch. Pull form over the
// IN-edge CSR: next[v] = (OR frontier[u] over in-neighbours u) & ~visited[v],
// visited[v] |= next[v]. frontier is read-only during the launch and a thread
// writes only next[v] and visited[v] of its own v. A vertex every source of
// the batch (full_mask) has reached skips its row.
//
// level_count[b] += vertices newly reached by source b in this level: each
// wave counts its rows bit by bit with ballots (lane b keeps the count of
// bit b), the waves of a block add into 64 LDS integer counters, and the
// block issues one integer atomicAdd per non-zero counter. Integer sums do
// not depend on order.
// ---------------------------------------------------------------------------
__global__ void k_msbfs_level(const long long* __restrict__ row_ptr,
                              const int* __restrict__ col_idx,
                              const u64* __restrict__ frontier,
                              u64* __restrict__ visited,
                              u64* __restrict__ next,
                              u64* __restrict__ level_count,
                              long long n, u64 full_mask) {
  __shared__ unsigned int cnt[WAVE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  if (threadIdx.x < WAVE) cnt[threadIdx.x] = 0;
  __syncthreads();
  unsigned int mine = 0;  // vertices this wave newly reached for bit `lane`
  const long long w0 = (long long)blockIdx.x * (blockDim.x / WAVE) + wid;
  const long long tw = (long long)gridDim.x * (blockDim.x / WAVE);
  for (long long b = w0 * WAVE; b < n; b += tw * WAVE) {
    const long long row = b + lane;
    long long s = 0, e = 0;
    u64 vis = full_mask;
    if (row < n) {
      vis = visited[row];
      s = row_ptr[row];
      e = row_ptr[row + 1];
    }
    const bool open = row < n && vis != full_mask;
    const bool longrow = open && (e - s) > WAVE;
    u64 nw = 0;
    if (open && !longrow) {
      u64 acc = 0;
      for (long long j = s; j < e; ++j) acc |= frontier[col_idx[j]];
      nw = acc & ~vis;
    }
    u64 mask = __ballot(longrow);
    while (mask) {
      const int bit = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const long long lrow = b + bit;
      const long long ls = row_ptr[lrow], le = row_ptr[lrow + 1];
      u64 acc = 0;
      long long j = ls + lane;
      for (; j + (HUB_ILP - 1) * WAVE < le; j += HUB_ILP * WAVE) {
        int u[HUB_ILP];
        u64 f[HUB_ILP];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) u[k] = col_idx[j + k * WAVE];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) f[k] = frontier[u[k]];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) acc |= f[k];
      }
      for (; j < le; j += WAVE) acc |= frontier[col_idx[j]];
      acc = wave_reduce_or(acc);
      if (lane == bit) nw = acc & ~vis;
    }
    if (row < n) {
      next[row] = nw;
      if (nw) visited[row] = vis | nw;
    }
    u64 any = wave_reduce_or(nw);
    while (any) {
      const int bit = __ffsll((long long)any) - 1;
      any &= any - 1;
      const unsigned int c = (unsigned int)__popcll(__ballot((nw >> bit) & 1));
      if (lane == bit) mine += c;
    }
  }
  if (mine) atomicAdd(&cnt[lane], mine);
  __syncthreads();
  if (threadIdx.x < WAVE && cnt[threadIdx.x])
    atomicAdd(&level_count[threadIdx.x], (u64)cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// Brandes forward sweep, one BFS level for a batch of sources. blockIdx.y is
// the source within the batch; dist / sigma are [B][n]. Pull over the
// IN-edge CSR: a vertex v with dist[v] == -1 sums sigma[u], in edge order,
// over its in-neighbours u with dist[u] == level; if there is one it takes
// dist[v] = level + 1 and sigma[v] = that sum.
//
// No atomics, and deterministic: during the launch the only writes to dist
// turn an entry from -1 into level + 1, so a concurrent read of an entry
// being written sees -1 or level + 1, never `level`. The set of u with
// dist[u] == level is therefore the same for every reader and fixed since
// the previous launch, and so is sigma[u] of those u (written by the launch
// that set dist[u] = level). dist[v] and sigma[v] are written by v's own
// thread (lane 0 of its wave for a hub row) and by nobody else.
// ---------------------------------------------------------------------------
__global__ void k_bc_forward(const long long* __restrict__ row_ptr,
                             const int* __restrict__ col_idx,
                             int* dist, double* sigma,
                             int* __restrict__ changed,
                             long long n, int level) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  dist += (long long)blockIdx.y * n;
  sigma += (long long)blockIdx.y * n;
  const long long w0 = (long long)blockIdx.x * (blockDim.x / WAVE) + wid;
  const long long tw = (long long)gridDim.x * (blockDim.x / WAVE);
  bool grew = false;
  for (long long b = w0 * WAVE; b < n; b += tw * WAVE) {
    const long long row = b + lane;
    const bool open = row < n && dist[row] == -1;
    long long s = 0, e = 0;
    if (open) {
      s = row_ptr[row];
      e = row_ptr[row + 1];
    }
    const bool longrow = (e - s) > WAVE;
    if (open && !longrow) {
      double acc = 0.0;
      bool hit = false;
      for (long long j = s; j < e; ++j) {
        const int u = col_idx[j];
        if (dist[u] == level) {
          acc += sigma[u];
          hit = true;
        }
      }
      if (hit) {
        sigma[row] = acc;
        dist[row] = level + 1;
        grew = true;
      }
    }
    u64 mask = __ballot(longrow);
    while (mask) {
      const int bit = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const long long lrow = b + bit;
      const long long ls = row_ptr[lrow], le = row_ptr[lrow + 1];
      double acc = 0.0;
      bool hit = false;
      long long j = ls + lane;
      // sigma is read whether or not dist matches, so that the gathers of
      // HUB_ILP edges are in flight together; a value that does not count is
      // dropped (it may be one that is being written this level)
      for (; j + (HUB_ILP - 1) * WAVE < le; j += HUB_ILP * WAVE) {
        int u[HUB_ILP], d[HUB_ILP];
        double sg[HUB_ILP];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) u[k] = col_idx[j + k * WAVE];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) d[k] = dist[u[k]];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) sg[k] = sigma[u[k]];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) {
          if (d[k] == level) {
            acc += sg[k];
            hit = true;
          }
        }
      }
      for (; j < le; j += WAVE) {
        const int u = col_idx[j];
        if (dist[u] == level) {
          acc += sigma[u];
          hit = true;
        }
      }
      acc = wave_reduce_sum_f64(acc);
      if (__ballot(hit) != 0 && lane == 0) {
        sigma[lrow] = acc;
        dist[lrow] = level + 1;
        grew = true;
      }
    }
  }
  if (grew) *changed = 1;
}

// ---------------------------------------------------------------------------
// Brandes backward sweep, one level for a batch of sources. Pull over the
// OUT-edge CSR: a vertex v with dist[v] == level takes
//   delta[v] = sum sigma[v] / sigma[w] * (1 + delta[w])
// over its out-neighbours w with dist[w] == level + 1, in edge order. Run
// from the deepest level down to 0. dist and sigma are read-only here; the
// delta[w] read were written by the launch of level + 1 and delta[v] is
// written by v's own thread only.
// ---------------------------------------------------------------------------
__global__ void k_bc_backward(const long long* __restrict__ row_ptr,
                              const int* __restrict__ col_idx,
                              const int* __restrict__ dist,
                              const double* __restrict__ sigma,
                              double* delta, long long n, int level) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  dist += (long long)blockIdx.y * n;
  sigma += (long long)blockIdx.y * n;
  delta += (long long)blockIdx.y * n;
  const long long w0 = (long long)blockIdx.x * (blockDim.x / WAVE) + wid;
  const long long tw = (long long)gridDim.x * (blockDim.x / WAVE);
  for (long long b = w0 * WAVE; b < n; b += tw * WAVE) {
    const long long row = b + lane;
    const bool mine = row < n && dist[row] == level;
    long long s = 0, e = 0;
    if (mine) {
      s = row_ptr[row];
      e = row_ptr[row + 1];
    }
    const bool longrow = (e - s) > WAVE;
    if (mine && !longrow) {
      const double sv = sigma[row];
      double acc = 0.0;
      for (long long j = s; j < e; ++j) {
        const int w = col_idx[j];
        if (dist[w] == level + 1) acc += sv / sigma[w] * (1.0 + delta[w]);
      }
      delta[row] = acc;
    }
    u64 mask = __ballot(longrow);
    while (mask) {
      const int bit = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const long long lrow = b + bit;
      const long long ls = row_ptr[lrow], le = row_ptr[lrow + 1];
      const double sv = sigma[lrow];
      double acc = 0.0;
      long long j = ls + lane;
      for (; j + (HUB_ILP - 1) * WAVE < le; j += HUB_ILP * WAVE) {
        int w[HUB_ILP], d[HUB_ILP];
        double sg[HUB_ILP], dl[HUB_ILP];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) w[k] = col_idx[j + k * WAVE];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) d[k] = dist[w[k]];
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k) {
          sg[k] = sigma[w[k]];
          dl[k] = delta[w[k]];
        }
#pragma unroll
        for (int k = 0; k < HUB_ILP; ++k)
          if (d[k] == level + 1) acc += sv / sg[k] * (1.0 + dl[k]);
      }
      for (; j < le; j += WAVE) {
        const int w = col_idx[j];
        if (dist[w] == level + 1) acc += sv / sigma[w] * (1.0 + delta[w]);
      }
      acc = wave_reduce_sum_f64(acc);
      if (lane == 0) delta[lrow] = acc;
    }
  }
}

// bc[v] += delta[b][v] for b = 0..B-1 in that order, skipping v == sources[b]:
// the sequential order makes the sum independent of the batch size.
__global__ void k_bc_accumulate(const double* __restrict__ delta,
                                const long long* __restrict__ sources,
                                double* __restrict__ bc, long long n, int nb) {
  long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; v < n; v += stride) {
    double acc = bc[v];
    for (int b = 0; b < nb; ++b)
      if (sources[b] != v) acc += delta[(long long)b * n + v];
    bc[v] = acc;
  }
}

// ===========================================================================
// Host wrappers
// ===========================================================================

static inline hipStream_t c_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// Checks the CSR pair and returns n.
static long long check_csr_n(const at::Tensor& row_ptr,
                             const at::Tensor& col_idx) {
  TORCH_CHECK(row_ptr.is_cuda() && row_ptr.scalar_type() == at::kLong &&
              row_ptr.is_contiguous() && row_ptr.dim() == 1 &&
              row_ptr.numel() >= 1,
              "row_ptr must be contiguous int64 CUDA [n+1]");
  TORCH_CHECK(col_idx.is_cuda() && col_idx.scalar_type() == at::kInt &&
              col_idx.is_contiguous() && col_idx.dim() == 1,
              "col_idx must be contiguous int32 CUDA [m]");
  TORCH_CHECK(col_idx.get_device() == row_ptr.get_device(),
              "row_ptr and col_idx must be on one device");
  return row_ptr.numel() - 1;
}

static void check_state(const at::Tensor& t, at::ScalarType ty,
                        std::initializer_list<long long> shape,
                        const at::Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.get_device() == like.get_device(), name,
              " must be a CUDA tensor on the graph's device");
  TORCH_CHECK(t.scalar_type() == ty, name, " has the wrong dtype");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == (long long)shape.size(), name,
              " has the wrong number of dimensions");
  int d = 0;
  for (long long want : shape) {
    TORCH_CHECK(t.size(d) == want, name, " has the wrong length: dim ", d,
                " is ", t.size(d), ", expected ", want);
    ++d;
  }
}

static int row_blocks(long long n) {
  return (int)std::max<long long>(
      std::min<long long>((n + 255) / 256, 16384), 1);
}

void msbfs_level(at::Tensor in_row_ptr, at::Tensor in_col_idx,
                 at::Tensor frontier, at::Tensor visited, at::Tensor next,
                 at::Tensor level_count, long long full_mask) {
  const long long n = check_csr_n(in_row_ptr, in_col_idx);
  check_state(frontier, at::kLong, {n}, in_row_ptr, "frontier");
  check_state(visited, at::kLong, {n}, in_row_ptr, "visited");
  check_state(next, at::kLong, {n}, in_row_ptr, "next");
  check_state(level_count, at::kLong, {WAVE}, in_row_ptr, "level_count");
  TORCH_CHECK(frontier.data_ptr() != next.data_ptr() &&
              frontier.data_ptr() != visited.data_ptr() &&
              visited.data_ptr() != next.data_ptr(),
              "frontier, visited and next must be distinct tensors");
  hipLaunchKernelGGL(
      k_msbfs_level, dim3(row_blocks(n)), dim3(256), 0, c_stream(),
      reinterpret_cast<const long long*>(in_row_ptr.data_ptr<int64_t>()),
      in_col_idx.data_ptr<int>(),
      reinterpret_cast<const u64*>(frontier.data_ptr<int64_t>()),
      reinterpret_cast<u64*>(visited.data_ptr<int64_t>()),
      reinterpret_cast<u64*>(next.data_ptr<int64_t>()),
      reinterpret_cast<u64*>(level_count.data_ptr<int64_t>()), n,
      (u64)full_mask);
  HIP_CHECK_LAST();
}

// The batch size of a [B][n] state tensor; B is blockIdx.y, so at most 65535.
static long long batch_of(const at::Tensor& dist) {
  TORCH_CHECK(dist.dim() == 2 && dist.size(0) >= 1 && dist.size(0) <= 65535,
              "dist must be [B][n] with 1 <= B <= 65535");
  return dist.size(0);
}

void bc_forward(at::Tensor in_row_ptr, at::Tensor in_col_idx, at::Tensor dist,
                at::Tensor sigma, at::Tensor changed, long long level) {
  const long long n = check_csr_n(in_row_ptr, in_col_idx);
  const long long nb = batch_of(dist);
  check_state(dist, at::kInt, {nb, n}, in_row_ptr, "dist");
  check_state(sigma, at::kDouble, {nb, n}, in_row_ptr, "sigma");
  check_state(changed, at::kInt, {1}, in_row_ptr, "changed");
  TORCH_CHECK(level >= 0 && level < 0x7fffffff, "level out of range");
  hipLaunchKernelGGL(
      k_bc_forward, dim3(std::min(row_blocks(n), 2048), (unsigned)nb),
      dim3(256), 0, c_stream(),
      reinterpret_cast<const long long*>(in_row_ptr.data_ptr<int64_t>()),
      in_col_idx.data_ptr<int>(), dist.data_ptr<int>(),
      sigma.data_ptr<double>(), changed.data_ptr<int>(), n, (int)level);
  HIP_CHECK_LAST();
}

void bc_backward(at::Tensor row_ptr, at::Tensor col_idx, at::Tensor dist,
                 at::Tensor sigma, at::Tensor delta, long long level) {
  const long long n = check_csr_n(row_ptr, col_idx);
  const long long nb = batch_of(dist);
  check_state(dist, at::kInt, {nb, n}, row_ptr, "dist");
  check_state(sigma, at::kDouble, {nb, n}, row_ptr, "sigma");
  check_state(delta, at::kDouble, {nb, n}, row_ptr, "delta");
  TORCH_CHECK(level >= 0 && level < 0x7fffffff, "level out of range");
  hipLaunchKernelGGL(
      k_bc_backward, dim3(std::min(row_blocks(n), 2048), (unsigned)nb),
      dim3(256), 0, c_stream(),
      reinterpret_cast<const long long*>(row_ptr.data_ptr<int64_t>()),
      col_idx.data_ptr<int>(), dist.data_ptr<int>(),
      sigma.data_ptr<double>(), delta.data_ptr<double>(), n, (int)level);
  HIP_CHECK_LAST();
}

void bc_accumulate(at::Tensor delta, at::Tensor sources, at::Tensor bc) {
  TORCH_CHECK(bc.is_cuda() && bc.scalar_type() == at::kDouble &&
              bc.is_contiguous() && bc.dim() == 1,
              "bc must be contiguous float64 CUDA [n]");
  const long long n = bc.numel();
  TORCH_CHECK(delta.dim() == 2 && delta.size(0) >= 1,
              "delta must be [B][n]");
  const long long nb = delta.size(0);
  TORCH_CHECK(nb <= 0x7fffffff, "batch too large");
  check_state(delta, at::kDouble, {nb, n}, bc, "delta");
  check_state(sources, at::kLong, {nb}, bc, "sources");
  const int blocks =
      (int)std::max<long long>(std::min<long long>((n + 255) / 256, 2048), 1);
  hipLaunchKernelGGL(
      k_bc_accumulate, dim3(blocks), dim3(256), 0, c_stream(),
      delta.data_ptr<double>(),
      reinterpret_cast<const long long*>(sources.data_ptr<int64_t>()),
      bc.data_ptr<double>(), n, (int)nb);
  HIP_CHECK_LAST();
}

// Fused MFMA score + top-k kNN kernel for large query batches.
//
// scores = DB[N,D] (bf16, row-major) x Q^T  with Q [BN,D] (bf16, row-major,
// padded to BN=256 queries), k-selection fused into the epilogue so the
// [N, Q] score matrix is never materialized in HBM. The DB shard is read
// exactly once per query batch.
//
// Structure (history of the measurements: profiles/README.md):
//   * a workgroup is KNN_RG row groups of KNN_BM = 160 corpus rows, four
//     waves each: wave w owns row group w >> 2 and query quarter w & 3
//     (64 columns), a 160x64 accumulator tile (233 VGPRs, no spills). The
//     panel is KNN_RG * 160 rows. KNN_RG = 2 (default): 8 waves, 320x256
//     output tile, one workgroup per CU. KNN_RG = 1: 4 waves, 160x256, two
//     workgroups per CU. Either way a CU holds 320 x 256 fp32 accumulators
//     in 8 waves; what differs is how often the query tile is staged.
//     The kernel is bound by what a CU can ingest: every corpus byte (HBM)
//     drags 256*2/panel bytes of query tile (L2) through the same load
//     path, 2.67 B at 96 rows, 1.6 B at 160, 0.8 B at 320. With KNN_RG = 2
//     both row groups read one staged copy of the query stage where two
//     independent workgroups each staged their own.
//     KNN_STAGGER = 1 (default, KNN_RG = 2 only): row group 1 runs half
//     a stage behind row group 0, so that on every SIMD one wave's MFMAs
//     run beside its partner's loads, waits and epilogue ("Pipeline
//     ordering, staggered form" below). Same scores and indices.
//   * one flat stream of BK=32 stages per workgroup: the (panel, k) loops
//     are flattened, stage g = (panel, 32-wide K slice). Per stage a wave
//     runs 40 mfma_f32_16x16x32_bf16 (ascending k per accumulator, the
//     same order as a BK=64 loop, so scores do not depend on the staging
//     or on KNN_RG).
//   * LDS (one array): query tile double-buffered (2 x 16 KB), corpus tile
//     in a ring of three buffers of panel x 64 B (20 KB at 320 rows), then
//     the epilogue region, 4 KB per wave: 124 KB at KNN_RG = 2, 78 KB at
//     KNN_RG = 1. Staged by __builtin_amdgcn_global_load_lds width 16.
//     While stage g computes, the queries of stage g+1 (L2-resident) and
//     the corpus rows of stages g+1 and g+2 (the HBM stream) are in
//     flight; the corpus prefetch crosses the panel boundary, so it also
//     runs under the top-k epilogue.
//   * stage rows are 64 B; 16 B-slot XOR swizzle, applied to the global
//     source address and to the ds_read address (see swz()).
//   * fragment reads and the epilogue's LDS traffic are inline asm with
//     explicit lgkmcnt waits and raw s_barrier: with compiler-visible LDS
//     accesses or __syncthreads() hipcc waits vmcnt(0) while an LDS-DMA is
//     outstanding and the prefetch drains every stage.
//   * transposed epilogue: acc fragments go 16 rows at a time through a
//     [col][16] fp32 block; each thread owns one (row group, query column)
//     pair and keeps a register top-K list (statically unrolled insertion).
//     The epilogue has no barrier (see "Epilogue privacy" below).
//   * corpus loads use the default cache policy: non-temporal (aux = 2)
//     measured 22 % slower (81.8 vs 67.1 ms at 100M rows, 96-row tile).
//
// Pipeline ordering, lockstep form (KNN_STAGGER = 0, and KNN_RG = 1). VM
// loads retire in order; counts are per wave, W = 4 * KNN_RG waves; numbers
// for W = 8, in brackets for W = 4:
//   stage g issues  B(g+1)  NB = 2 [4] instructions  -> sB[(g+1)&1]
//          then     A(g+2)  NA = 3 instructions      -> sA[(g+2)%3]
//   (NB = 256 query rows / 16 rows per 1 KB piece / W waves; NA = panel/16
//   pieces over W waves: 20 [10] pieces = 2 whole pieces per wave + one
//   8-row half piece per wave)
//   and ends with   s_waitcnt vmcnt(NA); s_barrier.
//   At that wait the wave's queue holds, oldest first,
//     A(g+1)[3] (issued in stage g-1, after B(g)), B(g+1)[2 or 4], A(g+2)[3],
//   everything older having been retired by stage g-1's wait. vmcnt(NA) =
//   vmcnt(3) therefore retires A(g+1) and B(g+1) and leaves exactly A(g+2)
//   in flight, whatever NB is. An A(g+1)-before-B(g) order would need a
//   wait that also drains the newest prefetch; issuing the prefetch LAST
//   is what keeps it in flight.
//   Read-after-DMA: stage g+1 reads sB[(g+1)&1] and sA[(g+1)%3] after the
//   barrier that follows that wait in every wave, so every wave's pieces
//   have landed (a wave reads query pieces staged by its partner wave of
//   the other row group, and corpus pieces staged by any wave). Write-
//   after-read: B(g+1) and A(g+2) overwrite the buffers stage g-1 read;
//   every wave retired those ds_reads (lgkmcnt(0) ahead of its last MFMA
//   group) before it arrived at stage g-1's end barrier, and a wave issues
//   stage g's loads only after it has left that barrier.
//
// Pipeline ordering, staggered form (KNN_STAGGER = 1 with KNN_RG = 2). Row
// group 0 (waves 0-3, the leader) and row group 1 (waves 4-7, the
// follower; wave w and w+4 share a SIMD) run the same stage program half a
// stage apart, so that one partner's MFMAs run beside the other's DMA
// issue, fragment reads, waits and epilogue. A stage is two segments, each
// ended by a workgroup s_barrier:
//   L(g)  issue the prefetch DMAs; read the 4 B fragments and the first
//         AH = 5 A fragments of stage g; s_waitcnt lgkmcnt(AH): LDS returns
//         in order, so the 4 B reads (issued first) are back; s_barrier.
//   C(g)  the MFMA ladder (10 groups of 4, the other 5 A reads interleaved
//         behind counted lgkmcnt, the last group behind lgkmcnt(0));
//         s_waitcnt vmcnt(NA); s_barrier.
//   Number the barrier intervals t = 0, 1, ... from the prologue's barrier.
//   The leader runs L(g) in t = 2g and C(g) in t = 2g+1; the follower takes
//   one extra barrier behind the prologue (it sits out t = 0) and runs L(g)
//   in t = 2g+1 and C(g) in t = 2g+2. Both run the same loop body; only the
//   extra barrier and who stages the queries differ.
//   Staging. Each row group's four waves stage that group's own 160 rows
//   of the corpus stage: 10 pieces = 2 whole pieces + one 8-row half piece
//   per wave, NA = 3 as before, into the group's half of sA[.] (offset
//   rowgroup * 160 * 64 B, the half its own fragments are read from). The
//   leader's four waves stage the whole query stage, NB = 4 pieces each,
//   ahead of their A pieces; follower waves issue no query DMA.
//   Queue at the vmcnt(3) that ends C(g), oldest first:
//     leader    A(g+1)[3], B(g+1)[4], A(g+2)[3]
//     follower  A(g+1)[3], A(g+2)[3]
//   everything older having been retired by C(g-1)'s wait; vmcnt(3) retires
//   all but A(g+2) in both. The prologue issues A(0), B(0) (leader), A(1)
//   and waits vmcnt(3): A(0) and B(0) have landed before its barrier.
//   sA[j], one row group's half (ring of 3, private to the group's waves):
//     written by the group's A(g+2) DMA, issued in its L(g), j = (g+2)%3;
//     read by the group's waves in L(g+2) (first 5 fragments) and C(g+2).
//     Read-after-DMA: each wave's vmcnt(3) at the end of C(g+1) retires its
//     A(g+2) pieces, the barrier behind it makes that hold for the group's
//     four waves, and L(g+2) lies behind that barrier.
//     Write-after-read: the half was last read in the group's C(g-1), whose
//     ladder ends with lgkmcnt(0) ahead of the barrier that ends C(g-1);
//     the group's L(g) lies behind that barrier. The other group never
//     touches this half, so its skew does not enter.
//   sB[j] (double buffer, shared by both groups):
//     written by the leader's B(g+1) DMA, issued in its L(g), t = 2g,
//     j = (g+1)&1; read only in L segments (all 4 B fragments of a stage
//     are read there and kept in registers through C): by the leader in
//     L(g+1), t = 2g+2, and by the follower in L(g+1), t = 2g+3.
//     Read-after-DMA: the leader's vmcnt(3) at the end of C(g), t = 2g+1,
//     retires B(g+1) ahead of the barrier that ends t = 2g+1; both readers
//     lie behind that barrier, one and two intervals later.
//     Write-after-read: sB[(g+1)&1] held stage g-1. Its last reader is the
//     follower's L(g-1) in t = 2g-1, whose lgkmcnt(AH) retires the B reads
//     ahead of the barrier that ends t = 2g-1; the leader's L(g) lies behind
//     that barrier (the leader's own L(g-1) was t = 2g-2).
//   Barriers per wave over a stream of G stages: 1 (prologue) + 2G + 1 in
//   both groups: the follower's extra one directly behind the prologue, the
//   leader's behind its last epilogue, where it closes the interval of the
//   follower's C(G-1). Panel boundaries add none: the epilogue is barrier-
//   free and the stage stream runs on, so the leader's epilogue falls into
//   the interval of the follower's last C of the panel and the follower's
//   into that of the leader's C of the next panel's first stage. A skipped
//   panel (filtered kernel) never enters the stream and adds none either;
//   next_live() reads the whole panel's mask words in every wave, so both
//   groups walk the same panel sequence. A workgroup without a live panel
//   takes no barrier at all (block-uniform branch).
//
//   Epilogue privacy: wave w writes its accumulator chunk to
//   [EPI_OFF + w*EPI_SLICE, +EPI_SLICE) and its own 64 lanes read one 64 B
//   row each of exactly that slice; no LDS-DMA ever targets the region. A
//   wave's LDS instructions execute in order and each chunk's writes and
//   reads are followed by lgkmcnt(0), so write -> read -> next chunk's
//   write is ordered inside the wave and no other wave is involved: the
//   epilogue needs no barrier. Waves drift through it independently; one
//   that finishes early runs on into the next panel's first stage, whose
//   operands were gated by the last stage's end barrier and whose
//   prefetches overwrite only buffers every wave finished reading before
//   that barrier. It then waits at that stage's end barrier, so no wave
//   gets more than one stage ahead of another (staggered: at the barrier
//   that ends the first stage's L segment, so the two groups keep their
//   half-stage distance and no wave gets a segment ahead within a group).
//   The filtered kernel finds the next panel with an allowed row before
//   the stage loop of the current one, so a skipped panel never enters the
//   stream: buffer rotation and outstanding-load counts do not see it.
//   At the end of the stream the prefetches are still issued (from the
//   current panel's rows, never used) to keep the counts uniform, and a
//   vmcnt(0) ahead of the candidate write-out retires them. They target
//   ring buffers only, under the same write-after-read argument as any
//   other stage's, and the LDS is released when the last wave has ended.
//
// Row bias (BIASED): the score that enters the top-k is dot + row_bias[r],
// r the local row (before row_base), added in the epilogue where a thread
// takes v[j>>2][j&3] for row grow0 + j: one fp32 add behind the finished
// dot product. All 64 lanes of a wave look at the same 16 rows of a chunk,
// so the 16 biases are wave-uniform and are fetched with scalar loads
// (plain C++ on a wave-uniform address: one s_load_dwordx16 per chunk, the
// add takes the SGPR as an operand; no VGPR, no VM-queue entry). Chunk 0's
// are fetched at the panel's start, beside the filtered kernel's mask
// words; chunk m+1's during chunk m, into the other of two 16-SGPR buffers
// (behind chunk m's LDS round trip rather than ahead of it, so that the
// load runs under chunk m's insertion pass instead of in front of a
// lgkmcnt(0)). Why this is safe in this pipeline:
//   * vmcnt is untouched: the loads are SMEM, the wait_vm<NA> accounting of
//     the stage stream sees nothing new, and no prefetch is drained.
//   * lgkmcnt: SMEM and LDS share the counter and SMEM may return out of
//     order. With u scalar loads outstanding at a counted wait_lgkm<N>, at
//     least issued_lds + u - N operations have completed, of which at most
//     u are scalar, so at least issued_lds - N LDS operations have: the
//     wait guarantees what it guaranteed, it can only take longer (chunk
//     0's load during the first stage; the mask words already live with
//     this). Their data is needed only in the epilogue, behind lgkmcnt(0).
//   * first use: chunk m+1's load is issued behind chunk m's second
//     lgkmcnt(0); chunk m+1's own two lgkmcnt(0) waits retire it ahead of
//     chunk m+1's first add, and chunk m reads the other buffer. The
//     compiler counts the load itself as well and puts its own lgkmcnt(0)
//     ahead of the first add.
//   * padding columns: a zero query column scores the bare bias, so with
//     fewer than BN real queries the padding columns' lists are closed at
//     the start (threshold 3e38, q_count argument); unbiased they score 0
//     everywhere and stop inserting by themselves.
//   * bounds: the last element read is row_bias[prow + rg*HM + HM - 1] with
//     prow + BM <= n_panels * BM = the length the wrapper checked. The
//     end-of-stream prefetch of an unused panel touches no bias.
// Biases must be finite and far above the -1e30 list sentinel; the kernel
// does not test for that.
//
// Replaces the reference's cublasSgemv + single-thread top-k scan
// (reference: pkg/gpu/cuda/cuda_kernels.cu:340-480).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <type_traits>
#include "common.h"
#include "allow_mask.h"
#include "topk.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define G_AS __attribute__((address_space(1)))
#define L_AS __attribute__((address_space(3)))

// tile geometry
#ifndef KNN_BM
#define KNN_BM 160  // rows of one row group (one wave's accumulator tile)
#endif
#ifndef KNN_RG
#define KNN_RG 2  // row groups per workgroup
#endif
static_assert(KNN_RG == 1 || KNN_RG == 2, "KNN_RG is 1 or 2");
#ifndef KNN_STAGGER
#define KNN_STAGGER 1  // row group 1 runs half a stage behind row group 0
#endif
static_assert(KNN_STAGGER == 0 || KNN_STAGGER == 1, "KNN_STAGGER is 0 or 1");
// the stagger needs two row groups in one workgroup; KNN_RG = 1 ignores it
#define KNN_STAG (KNN_STAGGER == 1 && KNN_RG == 2)
#define HM KNN_BM           // rows per row group
#define BM (KNN_RG * HM)    // rows per panel
#define BN 256
#define BK 32  // K extent of one pipeline stage
#define NWAVES (4 * KNN_RG)
#define NTHREADS (64 * NWAVES)
#define KCAND 10
#define MW (HM / 16)

#define SB_BYTES (BN * BK * 2)  // one query stage: 16 KB
#define SA_BYTES (BM * BK * 2)  // one corpus stage: 20 KB at BM=320
// epilogue: one [64 cols][16 rows] fp32 block per wave, behind the rings
#define EPI_SLICE (64 * 16 * 4)
#define EPI_OFF (2 * SB_BYTES + 3 * SA_BYTES)
#define EPI_BYTES (NWAVES * EPI_SLICE)
#define SMEM_BYTES (EPI_OFF + EPI_BYTES)
// Epilogue privacy (see header): a wave's four ds_write_b128 (offsets
// nn * 1024, lane part < 1024) cover exactly its slice, its 64 lanes read
// one 64 B row each of the same slice, and the region holds one slice per
// wave behind every DMA target.
static_assert(EPI_SLICE == 4 * (16 * 64),
              "a wave's four ds_write_b128 (16 cols x 64 B each) fill a slice");
static_assert(EPI_SLICE == WAVE * 64,
              "a wave's lanes read one 64 B row each of the same slice");
static_assert(EPI_OFF >= 2 * SB_BYTES + 3 * SA_BYTES &&
                  EPI_OFF + NWAVES * EPI_SLICE <= SMEM_BYTES,
              "one slice per wave, behind every LDS-DMA target");

// LDS-DMA instructions per wave per stage. A staging set is SWAVES waves
// that share one staging job: all NWAVES waves stage the whole panel and
// the query tile, or, staggered, each row group's four waves stage that
// group's A_ROWS = HM rows and row group 0's four waves the query tile. A
// set's corpus stage is A_ROWS/16 pieces of 1 KB (16 rows x 64 B); each
// wave stages A_FULL whole pieces and, when half a wave count of pieces is
// left over, one half piece (8 rows, lanes 0-31).
#if KNN_STAG
#define SWAVES 4
#define A_ROWS HM
#else
#define SWAVES NWAVES
#define A_ROWS BM
#endif
#define A_PIECES (A_ROWS / 16)
#define A_FULL (A_PIECES / SWAVES)
#define A_HALF (A_PIECES % SWAVES == SWAVES / 2 ? 1 : 0)
#define NA (A_FULL + A_HALF)
#define NB (BN / 16 / SWAVES)
static_assert(A_PIECES % SWAVES == 0 || A_PIECES % SWAVES == SWAVES / 2,
              "corpus stage must split evenly over the waves");
static_assert(!KNN_STAG || (HM * BK * 2) % 512 == 0 &&
                               ((HM * BK * 2) & 256) == 0,
              "a row group's staging base keeps the swizzle bit clear");
// resident workgroups per CU the tile is sized for: 8 waves per CU
#define KNN_WGS (KNN_RG == 2 ? 1 : 2)
static_assert(SMEM_BYTES * KNN_WGS <= 160 * 1024, "LDS budget per CU");
static_assert(SMEM_BYTES <= 128 * 1024, "static LDS limit per workgroup");

namespace knn_mfma_detail {

// Stage-image swizzle (self-inverse). Rows are 64 B = four 16 B slots and
// a 256 B bank row holds four rows. ds_read_b128 is served in 16-lane
// groups, each made of the lanes of rows 0-3 and 12-15 of one slot plus
// the lanes of rows 4-11 of its neighbour slot (g, g^1). With slot ^=
// 2*(row>>2 & 1) the four rows r, r+4, r+8, r+12 that share a bank-row
// position (r&3) get the distinct slots {g, g^1^2, g^1, g^2}: 16 distinct
// 16 B positions per group, conflict-free.
__device__ __forceinline__ int swz(int b) {
  return b ^ (((b >> 8) & 1) << 5);
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// LDS byte addresses: addrspace(3) pointer values are byte offsets.
template <int OFF, class T>
__device__ __forceinline__ void ds_read128(T& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <int OFF>
__device__ __forceinline__ void ds_write128(unsigned addr, float4v v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF)
               : "memory");
}
// sched_barrier: hipcc otherwise moves register-only MFMA/VALU across an
// inline-asm wait.
template <int N>
__device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One wave-instruction of LDS-DMA: 16 B per lane from gbase + voff to the
// wave-uniform LDS address lds + lane * 16.
__device__ __forceinline__ void glds(const char* gbase, unsigned voff,
                                     char* lds) {
  __builtin_amdgcn_global_load_lds(
      (const G_AS unsigned int*)(gbase + voff), (L_AS unsigned int*)lds, 16, 0,
      0);
}

}  // namespace knn_mfma_detail

// FILTERED: `allow` is a packed row mask (bit r&31 of word r>>5 set = local
// row r may be returned); a row group is HM/32 whole words and a panel
// BM/32. FILTERED=false never touches `allow`.
// BIASED: the score that enters the top-k is dot(q, row) + row_bias[r] for
// local row r, one fp32 add in the epilogue (see "Row bias" in the header).
// BIASED=false never touches `row_bias`.
// cand_* are [gridDim.x * KNN_RG, BN, KCAND]: one list per (block, row
// group, query column).
template <bool FILTERED, bool BIASED>
__global__ __launch_bounds__(NTHREADS, KNN_WGS) void k_knn_mfma(
    const unsigned short* __restrict__ db, const unsigned short* __restrict__ qs,
    long long n_panels,  // number of full BM-row panels
    int d,               // inner dim, % 64 == 0
    long long row_base, float* __restrict__ cand_score,
    int* __restrict__ cand_idx, const unsigned int* __restrict__ allow,
    const float* __restrict__ row_bias,
    int q_count) {  // real queries; columns from q_count up are padding
  using namespace knn_mfma_detail;
  static_assert(!FILTERED || HM % 32 == 0,
                "filtered kNN needs whole mask words per row group");
  // One array for all LDS (a second __shared__ object makes hipcc wait
  // vmcnt(0) ahead of LDS reads): sB[2] at 0, sA[3] behind them, then the
  // epilogue slices.
  __shared__ __align__(16) char smem[SMEM_BYTES];

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);  // wave 0..W-1
  const int wc = wv & 3;   // query quarter: columns wc*64 .. wc*64+63
  const int rg = wv >> 2;  // row group: panel rows rg*HM .. rg*HM+HM-1

  // per-thread top-K state: this thread owns query column tid % BN of row
  // group rg.
  float tv[KCAND];
  int ti[KCAND];
  // topk_init() written out: with the helper hipcc allocates this kernel's
  // registers differently (10 more VGPRs unbiased), see NOTES.md
#pragma unroll
  for (int i = 0; i < KCAND; ++i) { tv[i] = -1e30f; ti[i] = -1; }
  if constexpr (BIASED) {
    // A padding column (zero query) scores the bare bias: distinct values
    // that would keep inserting like a real query's, where an unbiased
    // padding column scores 0 everywhere and stops after KCAND rows. Its
    // list is closed instead; the caller drops these columns.
    if (tid % BN >= q_count) {
#pragma unroll
      for (int i = 0; i < KCAND; ++i) tv[i] = 3e38f;
    }
  }

  const int d2 = d * 2;       // row stride in bytes
  const int nstage = d / BK;  // stages per panel, even and >= 2

  // first panel of this block that has an allowed row, from p upward
  auto next_live = [&](long long p) -> long long {
    if constexpr (FILTERED) {
      while (p < n_panels) {
        unsigned int any = 0;
#pragma unroll
        for (int h = 0; h < BM / 32; ++h) any |= allow[((p * BM) >> 5) + h];
        if (any != 0) break;
        p += gridDim.x;
      }
    }
    return p;
  };

  long long panel = next_live(blockIdx.x);
  if (panel < n_panels) {  // block-uniform
    // Staging: lane L of a piece covers LDS bytes x = L*16 (+ piece base, a
    // multiple of 512 with bit 8 clear), which hold logical bytes swz(x):
    // row x>>6, slot (L&3) ^ 2*((L>>4)&1). The per-lane source offset is
    // the same for every piece of either operand.
    const unsigned voff =
        (unsigned)((lane >> 2) * d2 +
                   (((lane & 3) ^ (((lane >> 4) & 1) << 1)) << 4));
    // Staging set (see SWAVES): wave sw of its set. Staggered, a row group
    // stages its own rows, arow0 .. arow0+HM-1 of the panel, which sit
    // arow0 * 64 B into a corpus buffer, and only row group 0 stages
    // queries; otherwise the one set is the workgroup.
    constexpr bool STAG = KNN_STAG;
    const int sw = STAG ? wc : wv;
    const int arow0 = STAG ? rg * HM : 0;
    // wave sw stages query pieces sw*NB .. sw*NB+NB-1 (16 rows each)
    const char* qbase = (const char*)qs + (long long)(sw * NB * 16) * d2;

    auto issue_b = [&](int s, int boff) {
      const char* g = qbase + s * (BK * 2);
#pragma unroll
      for (int c = 0; c < NB; ++c)
        glds(g + (long long)(c * 16) * d2, voff,
                smem + boff + (sw * NB + c) * 1024);
    };
    auto issue_a = [&](long long prow, int s, int aoff) {
      const char* g =
          (const char*)db + (prow + arow0) * d2 + s * (BK * 2);
      char* l = smem + aoff + arow0 * (BK * 2);
#pragma unroll
      for (int c = 0; c < A_FULL; ++c)
        glds(g + (long long)((sw * A_FULL + c) * 16) * d2, voff,
                    l + (sw * A_FULL + c) * 1024);
      if constexpr (A_HALF) {
        // last SWAVES/2 pieces as SWAVES 8-row halves, one per wave
        if (lane < 32)
          glds(g + (long long)(SWAVES * A_FULL * 16 + sw * 8) * d2, voff,
                      l + SWAVES * A_FULL * 1024 + sw * 512);
      }
    };

    // fragment (row r0 + lane%16, k-slot lane/16) at its swizzled position
    const unsigned foff = (unsigned)swz((lane & 15) * 64 + (lane >> 4) * 16);
    const unsigned lds0 = (unsigned)(unsigned long long)(L_AS char*)smem;
    const unsigned fb = lds0 + wc * (64 * BK * 2) + foff;  // + sB offset
    const unsigned fa = lds0 + rg * (HM * BK * 2) + foff;  // + sA offset
    // epilogue block [col][16] fp32, 64 B rows, slot ^= (col>>2)&3: the
    // column owner's float4 reads (one row per lane, same slot) spread a
    // 16-lane group over 16 distinct 16 B positions. Both addresses stay
    // inside this wave's slice at `eb`.
    const unsigned eb = lds0 + EPI_OFF + wv * EPI_SLICE;
    const unsigned ew = eb + (lane & 15) * 64 +
                        (((lane >> 4) ^ ((lane >> 2) & 3)) << 4);
    const unsigned er = lane * 64 + (((lane >> 2) & 3) << 4);  // slot 0, + eb

    int b_cur = 0, b_nxt = SB_BYTES;
    int a_cur = 2 * SB_BYTES, a_nxt = a_cur + SA_BYTES, a_nn = a_nxt + SA_BYTES;

    // prologue: A(0), B(0), A(1); gate the first two
    issue_a(panel * BM, 0, a_cur);
    if (!STAG || rg == 0) issue_b(0, b_cur);
    issue_a(panel * BM, 1, a_nxt);
    wait_vm<NA>();
    __builtin_amdgcn_s_barrier();
    if constexpr (STAG) {
      // the follower sits out interval 0: from here on it runs one
      // barrier interval (half a stage) behind the leader
      if (rg == 1) __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }

    for (;;) {
      const long long prow = panel * BM;
      // the skip decision for the following panel precedes its prefetch
      const long long nxt = next_live(panel + gridDim.x);
      const long long prow_pf = (nxt < n_panels ? nxt : panel) * BM;

      // mask words of this wave's row group
      unsigned int aw[(HM + 31) / 32];
      if constexpr (FILTERED) {
#pragma unroll
        for (int h = 0; h < HM / 32; ++h)
          aw[h] = allow[((prow + rg * HM) >> 5) + h];
      }
      // biases of this wave's row group, one 16-row chunk at a time, wave-
      // uniform (scalar loads): chunk 0 here, chunk m+1 in chunk m's epilogue
      const float* bias_rg = nullptr;
      float bz[2][16];
      if constexpr (BIASED) {
        bias_rg = row_bias + prow + rg * HM;
#pragma unroll
        for (int j = 0; j < 16; ++j) bz[0][j] = bias_rg[j];
      }

      float4v acc[MW][4];
#pragma unroll
      for (int m = 0; m < MW; ++m)
#pragma unroll
        for (int nn = 0; nn < 4; ++nn) acc[m][nn] = {0.f, 0.f, 0.f, 0.f};

      for (int s = 0; s < nstage; ++s) {
        // ---- prefetch: queries of the next stage, corpus two ahead ----
        if (!STAG || rg == 0) issue_b(s + 1 == nstage ? 0 : s + 1, b_nxt);
        {
          const bool wrap = s + 2 >= nstage;
          issue_a(wrap ? prow_pf : prow, wrap ? s + 2 - nstage : s + 2, a_nn);
        }

        // ---- fragments of this stage, then MFMA behind counted waits ----
        // Reads in consumption order: 4 B, the first AH A fragments, then
        // A fragment m+AH into the registers of fragment m once row group
        // m has issued its MFMAs (an MFMA reads its A/B operands at issue;
        // the read returns at least an LDS latency later). LDS returns in
        // order, so before group m the wave may leave outstanding
        //   issued(4 + AH + min(m, MW-AH)) - needed(5 + m).
        constexpr int AH = (MW + 1) / 2;
        bf16x8 bfr[4], afr[AH];
        const unsigned rb = fb + b_cur, ra = fa + a_cur;
        static_for<0, 4>([&](auto nn) {
          ds_read128<decltype(nn)::value * 1024>(bfr[decltype(nn)::value], rb);
        });
        static_for<0, AH>([&](auto m) {
          ds_read128<decltype(m)::value * 1024>(afr[decltype(m)::value], ra);
        });
        if constexpr (STAG) {
          // end of the load segment: the B fragments (the first four reads,
          // LDS returns in order) are back, so the query buffer is free for
          // the leader's next DMA; the AH A reads stay in flight
          wait_lgkm<AH>();
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(1);
        static_for<0, MW>([&](auto mc) {
          constexpr int m = decltype(mc)::value;
          constexpr int more = m < MW - AH ? m : MW - AH;
          wait_lgkm<AH - 1 + more - m>();
#pragma unroll
          for (int nn = 0; nn < 4; ++nn)
            acc[m][nn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afr[m % AH], bfr[nn], acc[m][nn], 0, 0, 0);
          if constexpr (m + AH < MW) {
            __builtin_amdgcn_sched_barrier(0);
            ds_read128<(m + AH) * 1024>(afr[m % AH], ra);
          }
        });
        __builtin_amdgcn_s_setprio(0);

        // retire A(g+1) and B(g+1); A(g+2) stays in flight (see header)
        wait_vm<NA>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        {
          int t = b_cur; b_cur = b_nxt; b_nxt = t;
          t = a_cur; a_cur = a_nxt; a_nxt = a_nn; a_nn = t;
        }
      }

      // ---- epilogue: 16-row chunks through this wave's transposed block;
      // no barrier, the slice is wave-private (see header) ----
      // the asm stores below read MFMA results: cover the MFMA-write ->
      // LDS-read wait states the compiler cannot see into the asm for
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      static_for<0, MW>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        static_for<0, 4>([&](auto nn) {
          ds_write128<decltype(nn)::value * 1024>(ew,
                                                  acc[m][decltype(nn)::value]);
        });
        wait_lgkm<0>();
        float4v v[4];
        static_for<0, 4>([&](auto sl) {
          ds_read128<0>(v[decltype(sl)::value],
                        eb + (er ^ (unsigned)(decltype(sl)::value << 4)));
        });
        wait_lgkm<0>();
        if constexpr (BIASED && m + 1 < MW) {
          // Next chunk's biases, behind this chunk's LDS round trip: the
          // load is in flight under the insertion pass below, and the next
          // chunk's first lgkmcnt(0) retires it ahead of its first use.
          // (Ahead of the ds_writes it would sit in front of that wait and
          // the wave would stall on it in every chunk.)
          // The empty asm reads one of THIS chunk's biases. hipcc does not
          // see the asm waits above and owes that load a lgkmcnt(0) of its
          // own ahead of the first use; SMEM returns out of order, so placed
          // behind the new load that wait would drain the new load too. The
          // read puts it here, where it is free.
          asm volatile("" ::"s"(bz[m & 1][0]));
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int j = 0; j < 16; ++j)
            bz[(m + 1) & 1][j] = bias_rg[(m + 1) * 16 + j];
        }
        const long long grow0 = prow + rg * HM + m * 16;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          float s = v[j >> 2][j & 3];
          if constexpr (BIASED) s += bz[m & 1][j];
          bool ok = s > tv[KCAND - 1];
          if constexpr (FILTERED)
            ok = ok && ((aw[m >> 1] >> ((m & 1) * 16 + j)) & 1u);
          if (ok) topk_insert(tv, ti, s, (int)(grow0 + j));
        }
        __builtin_amdgcn_sched_barrier(0);
      });

      if (nxt >= n_panels) break;
      panel = nxt;
    }
    if constexpr (STAG) {
      // the leader's last epilogue ran beside the follower's last compute
      // segment; this barrier closes that interval, so that every wave
      // has taken 2 + 2 * stages barriers
      if (rg == 0) __builtin_amdgcn_s_barrier();
    }
    // end of stream: retire the unused tail prefetches before the LDS goes
    wait_vm<0>();
  }

  // ---- write candidates: list (block * KNN_RG + rg), column tid % BN ----
  long long slot = (long long)blockIdx.x * (BN * KNN_RG) + tid;
#pragma unroll
  for (int i = 0; i < KCAND; ++i) {
    cand_score[slot * KCAND + i] = tv[i];
    cand_idx[slot * KCAND + i] = ti[i];
  }
}

// ---------------------------------------------------------------------------
// host wrapper: full-panel part of the shard only (n_panels * BM rows).
// The python side handles the tail rows and q-padding to 256.
// ---------------------------------------------------------------------------
template <bool FILTERED, bool BIASED>
static void launch_knn_mfma(int grid, hipStream_t stream, const at::Tensor& db,
                            const at::Tensor& q, long long n_panels, int d,
                            long long row_base, at::Tensor& cand_s,
                            at::Tensor& cand_i, const unsigned int* allow_p,
                            const float* bias_p, int q_count) {
  hipLaunchKernelGGL((k_knn_mfma<FILTERED, BIASED>), dim3(grid), dim3(NTHREADS),
                     0, stream, (const unsigned short*)db.data_ptr(),
                     (const unsigned short*)q.data_ptr(), n_panels, d, row_base,
                     cand_s.data_ptr<float>(), cand_i.data_ptr<int>(), allow_p,
                     bias_p, q_count);
}

std::tuple<at::Tensor, at::Tensor> knn_mfma(at::Tensor db, at::Tensor q,
                                            long long row_base, int k_out,
                                            c10::optional<at::Tensor> allow,
                                            c10::optional<at::Tensor> row_bias,
                                            int q_count) {
  TORCH_CHECK(db.is_cuda() && db.dim() == 2 && db.is_contiguous() &&
                  db.scalar_type() == at::kBFloat16,
              "knn_mfma: db must be contiguous 2D bf16 CUDA");
  TORCH_CHECK(q.is_cuda() && q.dim() == 2 && q.is_contiguous() &&
                  q.scalar_type() == at::kBFloat16,
              "knn_mfma: q must be contiguous 2D bf16 CUDA");
  long long n = db.size(0);
  int d = (int)db.size(1);
  TORCH_CHECK(q.size(0) == BN, "knn_mfma: q must be padded to ", BN, " rows");
  TORCH_CHECK(q.size(1) == d, "dim mismatch");
  TORCH_CHECK(d % 64 == 0, "knn_mfma needs D % 64 == 0");
  TORCH_CHECK(n % BM == 0, "knn_mfma needs N % ", BM, " == 0 (python pads/tails)");
  TORCH_CHECK(n < (1LL << 31), "shard too large for int32 local rows");
  TORCH_CHECK(k_out >= 1 && k_out <= KCAND);
  TORCH_CHECK(q_count >= 1 && q_count <= BN, "knn_mfma: q_count must be 1..",
              BN);
  const unsigned int* allow_p = nullptr;
  if (allow.has_value()) allow_p = check_allow_mask(*allow, db, n, "knn_mfma");
  const float* bias_p = nullptr;
  if (row_bias.has_value())
    bias_p = check_row_bias(*row_bias, db, n, "knn_mfma");

  long long n_panels = n / BM;
  // Persistent-style grid. Lockstep builds: 3 blocks per resident slot (256
  // CUs x KNN_WGS workgroups), so every dispatch wave is full: 768 at
  // KNN_RG = 2, 1536 at KNN_RG = 1. Each block walks many panels back to
  // back through one stage stream; its top-k thresholds tighten early and
  // the candidate buffers and the merge shrink with the grid. Swept at 100M
  // rows, KNN_RG = 2, lockstep: 1536 57.2 ms, 768 56.2, 512 55.8, 256 55.1;
  // end to end 256 and 768 were within each other's spread there. The
  // staggered build gains only with long-lived blocks (kernel, same box:
  // 768 55.5-56.0 ms against 55.7-56.0 lockstep, 512 55.0-55.2 against
  // 55.5-55.6, 256 54.2-54.6 against 55.0-55.3) and one block per CU wins
  // end to end by more than the runs' spread in two sessions, so its
  // default is 256 (profiles/README.md). NORNICDB_KNN_GRID overrides.
  int max_grid = KNN_STAG ? 256 : 256 * KNN_WGS * 3;
  if (const char* g = getenv("NORNICDB_KNN_GRID")) max_grid = atoi(g);
  int grid = (int)std::min<long long>(n_panels, max_grid);
  auto stream = at::hip::getCurrentHIPStream().stream();

  auto opts_f = db.options().dtype(at::kFloat);
  auto opts_i32 = db.options().dtype(at::kInt);
  auto opts_i64 = db.options().dtype(at::kLong);
  // one candidate list per (block, row group, query column)
  const long long n_lists = (long long)grid * KNN_RG;
  at::Tensor cand_s = at::empty({n_lists, BN, KCAND}, opts_f);
  at::Tensor cand_i = at::empty({n_lists, BN, KCAND}, opts_i32);

  auto launch = bias_p ? launch_knn_mfma<false, true>
                       : launch_knn_mfma<false, false>;
  if (allow_p != nullptr) {
#if KNN_BM % 32 == 0
    launch = bias_p ? launch_knn_mfma<true, true>
                    : launch_knn_mfma<true, false>;
#else
    TORCH_CHECK(false, "knn_mfma: filtered search needs KNN_BM % 32 == 0");
#endif
  }
  launch(grid, stream, db, q, n_panels, d, row_base, cand_s, cand_i, allow_p,
         bias_p, q_count);
  HIP_CHECK_LAST();

  at::Tensor out_s = at::empty({BN, k_out}, opts_f);
  at::Tensor out_i = at::empty({BN, k_out}, opts_i64);
  topk_merge(cand_s, cand_i, n_lists, BN, k_out, row_base, out_s, out_i,
             stream);
  return {out_s, out_i};
}

// panel height (rows the kernel route consumes at a time) and row groups
long long knn_bm_value() { return BM; }
long long knn_rg_value() { return KNN_RG; }
// 1 when the built kernel staggers its row groups (KNN_RG = 2 only)
long long knn_stagger_value() { return KNN_STAG ? 1 : 0; }

// Pipelined bf16 GEMM with fp32 output and deterministic split-K, for gfx950 (MI355X): the decoder's batched weight
// gradients dW = dY^T X and input gradients dX = dY W -- the autograd backward of the reference's nn.Linear /
// nn.LSTMCell weights (decoder.py:115,118-125,149-158, attention.py:15-16) that train.py:163's loss.backward() runs.
//
//   C[M,N] = A(m,k) . B(n,k) (+ add1[M,N]) (+ C when beta = 1)      bf16 in, fp32 accumulate, fp32 out
//   A(m,k) = AT ? A[k lda + m] : A[m lda + k];   B(n,k) = BT ? B[k ldb + n] : B[n ldb + k]
//
// These products have a long K (B (T-1) = 3,328 rows, or the vocabulary) and few output tiles (32-316), so most of
// them need split-K to fill 256 CUs.  Split-K by fp32 atomics into C (the tile kernel's form) is bound by the memory
// side's ~1.3 TB/s of added bytes (MI355X_MICROARCH.md, Global float atomics): 20-30 MB of atomics per product, as
// long as the GEMM itself.  Here:
//   * BM x 128 x 64 block tiles, BM = 256 (4 M x 2 N waves of 64 x 64) or 128 (2 x 4 waves of 64 x 32), one 8-wave
//     workgroup per CU; what bounds a tile is the bytes each CU's load path delivers (~45-50 GB/s per CU measured:
//     DESIGN.md 4.3), so the taller tile moves 25 % fewer bytes per FLOP and the planner below picks per shape;
//   * 3-stage LDS ring filled by buffer_load ... lds (16 B per lane; offsets past an operand's end read zeros, so K
//     tails and M / N edges need no branches), one counted vmcnt + raw s_barrier per k-tile with tile t+2 in
//     flight while t is consumed; k-major operands staged as 64 k-rows of 256 B and read by ds_read_b64_tr_b16
//     (cdna_hip_programming.md T10), m/n-major ones as 128-B rows read by ds_read_b128, both conflict-free;
//   * split-K without atomics: split s stores its fp32 partial tile, in the accumulator layout (1 KiB per wave
//     instruction), with write-through (sc1) stores into slab s of the caller's workspace, drains them, and takes
//     an agent-scope ticket; the workgroup that draws the last ticket adds the partials in split order 0, 1, ...,
//     S-1 (its own from registers, the others by sc1 loads) and writes C.  The sum does not depend on which split
//     finished last: bit-identical run to run.  Hand-off: the payload write-through (sc1) and drained by every storing
//     wave, a barrier, an agent-scope release + relaxed ticket add by one lane; the last adder takes an agent-scope
//     acquire before its sc1 loads (cdna_hip_programming.md Guideline 16: a release / acquire pair under the memory
//     model, besides the sc1 form MI355X_MICROARCH.md measures valid on its own);
//   * XCD-aware order: the n-tiles of one (split, m-tile) panel share an XCD's L2.
#include <algorithm>
#include <atomic>
#include <climits>
#include <map>
#include <mutex>
#include <optional>
#include <queue>
#include <vector>

#include "sat_common.h"
#include "sat_internal.h"
#include "sat_lds_pipe.h"

// The partial-tile hand-off without agent-scope fences: every partial is stored `sc1` (write-through, 16 B), every
// storing wave waits vmcnt(0) before the workgroup barrier, one lane per workgroup then adds to the tile's ticket
// (agent atomic), the workgroup whose add returned splits - 1 is the reader, and every load of the partials is a 16-B
// `sc1` buffer load issued after that add returned (the other waves after the barrier the adding wave joins): the
// first row of MI355X_MICROARCH.md's table of hand-offs measured valid with `sc1` loads in place of the acquire, whose
// condition (2) makes the release redundant too (one workgroup per CU, hipMalloc'd workspace).  The fences cost a
// `buffer_wbl2` / `buffer_inv` per tile: bench line 6.111-6.136 -> 6.069-6.088 ms with both hand-offs fence-free
// (profiles/r6_s65, with the attention backward's); 1 = the fenced forms (A/B builds).
#ifndef SAT_SPLIT_RELEASE
#define SAT_SPLIT_RELEASE 0
#endif
#ifndef SAT_SPLIT_ACQUIRE
#define SAT_SPLIT_ACQUIRE 0
#endif
#ifndef SAT_SPLIT_DEBUG    // diagnostics builds: 1 = record every ticket draw (tools/debug_split_tickets.py)
#define SAT_SPLIT_DEBUG 0
#endif
#if SAT_SPLIT_DEBUG
__device__ unsigned g_sdbg[1 << 20];
__device__ unsigned g_sdbg_n;
__device__ unsigned g_sdbg_cs[64 * 256];   // per (launch % 64, tile): XOR of the final tile's bits
static unsigned g_sdbg_launch = 0;
#endif

namespace {

constexpr int SBN = 128, SBK = 64, SNSTG = 3;
constexpr int kMaxSplits = 8;
constexpr int kSplitCUs = 256;   // one workgroup per CU: a split grid stays within one round

template <int BM>
struct SGeom {
  static constexpr int WGN = BM == 256 ? 2 : 4;   // waves along N
  static constexpr int WGM = 8 / WGN;
  static constexpr int WTM = BM / WGM, WTN = SBN / WGN;
  static constexpr int MI = WTM / 16, NJ = WTN / 16;
  static constexpr int STAGE_A = BM * SBK * 2, STAGE_B = SBN * SBK * 2, STAGE = STAGE_A + STAGE_B;
  static constexpr int AI = STAGE_A / 1024 / 8, BI = STAGE_B / 1024 / 8, INSTR = AI + BI;   // 1 KiB DMAs per wave
  static constexpr int EPI_LD = SBN + 4;
  static constexpr int EPI_BYTES = BM * EPI_LD * 4;
  static constexpr int LDS = SNSTG * STAGE;
  static_assert(WTM == 64 && MI == 4, "wave tiles are 64 rows high");
  static_assert(EPI_BYTES + 16 <= LDS, "epilogue tile + ticket word must fit in the ring");
};

struct SArgs {
  int M, N, K;
  const bf16* A; long lda;
  const bf16* B; long ldb;
  float* C; long ldc;
  int beta1;              // C += product (beta = 1)
  const float* add1; long ld_add1;   // fp32 addend (nullable)
  int splits, kchunk;     // split s: K range [s kchunk, min(K, (s + 1) kchunk)), kchunk a multiple of SBK
  int a_mlim;             // k-major A: 8-element chunks are read while m + 8 <= a_mlim (SatGemm::a_tail)
  int tiles_m, tiles_n;
  unsigned a_bytes, b_bytes, c_bytes, slab_bytes;
  float* slab;            // splits > 1: [tile][split][BM x SBN] partials in the accumulator layout
  unsigned* tickets;      // splits > 1: one arrival counter per tile, zero at launch
  SatStamps st;
  unsigned dbg_launch;    // SAT_SPLIT_DEBUG builds: launch number
};

// Block lin of a product's nwg = tiles_m x tiles_n x splits blocks -> its (m-tile, n-tile, split).  XCD-aware order
// (cdna_hip_programming.md T1, bijective form): each XCD takes a contiguous run of (split, m-tile, n-tile) indices,
// so the workgroups on one XCD share their A panel.  Host code (the planner's checks) shares the mapping.
__host__ __device__ __forceinline__ void split_block_work(int lin, int nwg, int tiles_m, int tiles_n, int* mt, int* nt,
                                                          int* split) {
  const int q = nwg / 8, r = nwg % 8, x = lin % 8;
  lin = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + lin / 8;
  *nt = lin % tiles_n;
  const int rest = lin / tiles_n;
  *mt = rest % tiles_m;
  *split = rest / tiles_m;
}

__device__ __forceinline__ uint4 f4u(f32x4 v) {
  return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}

// One workgroup's (tile, split) of product a: block lin of the product's nwg, on the caller's LDS ring smem
// (SGeom<BM>::LDS bytes, 16-B aligned).
template <int BM, bool AT, bool BT>
__device__ __forceinline__ void split_gemm_body(const SArgs& a, char* smem, int lin, const int nwg) {
  using G = SGeom<BM>;
  constexpr int MI = G::MI, NJ = G::NJ, AI = G::AI, BI = G::BI;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / G::WGN, wn = w % G::WGN;

  int mt, nt, split;
  split_block_work(lin, nwg, a.tiles_m, a.tiles_n, &mt, &nt, &split);
  const int m0 = mt * BM, n0 = nt * SBN;
  const int M = a.M, N = a.N;
  const int kbeg = split * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  const int nk = kend > kbeg ? (kend - kbeg + SBK - 1) / SBK : 0;

  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, (short)0, (int)a.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)a.B, (short)0, (int)a.b_bytes, 0x00020000);
  // per-lane DMA pieces, fixed across k-tiles: k-major (4 k-rows of 256 B per 1 KiB instruction: lane -> k-row
  // lane >> 4, slot lane & 15) or m/n-major (8 rows of 128 B: lane -> row lane >> 3, slot lane & 7); the element
  // offset without k, and the k-row / k-chunk the lane adds per tile
  int a_off[AI], a_k[AI];
  bool a_ok[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) {
    if constexpr (AT) {
      const int q = (w * AI + j) * 4 + (lane >> 4);   // half q >> 6 (128 m each), k-row q & 63
      const int kr = q & 63, ch = (lane & 15) ^ sat_swz256(kr);
      const int m = m0 + (q >> 6) * 128 + 8 * ch;
      a_ok[j] = m + 8 <= a.a_mlim;
      a_off[j] = m;
      a_k[j] = kr;
    } else {
      const int r = (w * AI + j) * 8 + (lane >> 3);
      const int ch = (lane & 7) ^ ((r >> 1) & 7);
      a_ok[j] = m0 + r < M;
      a_off[j] = (int)((long)(m0 + r) * a.lda);
      a_k[j] = 8 * ch;
    }
  }
  int b_off[BI], b_k[BI];
  bool b_ok[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    if constexpr (BT) {
      const int kr = (w * BI + j) * 4 + (lane >> 4), ch = (lane & 15) ^ sat_swz256(kr);
      const int n = n0 + 8 * ch;
      b_ok[j] = n + 8 <= N;
      b_off[j] = n;
      b_k[j] = kr;
    } else {
      const int r = (w * BI + j) * 8 + (lane >> 3);
      const int ch = (lane & 7) ^ ((r >> 1) & 7);
      b_ok[j] = n0 + r < N;
      b_off[j] = (int)((long)(n0 + r) * a.ldb);
      b_k[j] = 8 * ch;
    }
  }
  auto stage = [&](int buf, int k0) {
    char* sa = smem + buf * G::STAGE;
    char* sb = sa + G::STAGE_A;
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const int k = k0 + a_k[j];
      const bool ok = a_ok[j] && k < kend;
      const unsigned off = AT ? 2u * (unsigned)((long)k * a.lda + a_off[j]) : 2u * (unsigned)(a_off[j] + k);
      sat_bdma16(rA, sa + (w * AI + j) * 1024, ok ? off : kSatOOB);
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const int k = k0 + b_k[j];
      const bool ok = b_ok[j] && k < kend;
      const unsigned off = BT ? 2u * (unsigned)((long)k * a.ldb + b_off[j]) : 2u * (unsigned)(b_off[j] + k);
      sat_bdma16(rB, sb + (w * BI + j) * 1024, ok ? off : kSatOOB);
    }
  };

  // fragments of 32-deep half h of the tile in buf
  const int fr = lane & 15, fh = lane >> 4, sw = (fr >> 1) & 7;
  const int am = wm * G::WTM;   // the wave's first row in the tile
  auto frags = [&](int buf, int h, bf16x8 (&fa)[MI], bf16x8 (&fb)[NJ]) {
    const char* sa = smem + buf * G::STAGE;
    const char* sb = sa + G::STAGE_A;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if constexpr (AT) fa[i] = sat_frag_kmajor(sa + (am >> 7) * (64 * 256), h * 32, (am & 127) + i * 16, lane);
      else fa[i] = *(const bf16x8*)(sa + (am + i * 16 + fr) * 128 + 16 * ((h * 4 + fh) ^ sw));
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if constexpr (BT) fb[j] = sat_frag_kmajor(sb, h * 32, wn * G::WTN + j * 16, lane);
      else fb[j] = *(const bf16x8*)(sb + (wn * G::WTN + j * 16 + fr) * 128 + 16 * ((h * 4 + fh) ^ sw));
    }
  };
  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mfma = [&](const bf16x8 (&fa)[MI], const bf16x8 (&fb)[NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
  };

  bf16x8 xa[MI], xb[NJ], ya[MI], yb[NJ];
  if (nk > 0) {
    stage(0, kbeg);
    if (nk > 1) {
      stage(1, kbeg + SBK);
      sat_vm_lds_barrier<G::INSTR>();
    } else {
      sat_vm_lds_barrier<0>();
    }
    frags(0, 0, xa, xb);
    int cur = 0;
    for (int t = 0; t < nk; ++t) {
      frags(cur, 1, ya, yb);   // second half of tile t (its reads retire before this tile's barrier)
      __builtin_amdgcn_sched_barrier(0);
      // tile t+2 into the stage tile t-1 used: every wave's reads of it retired before tile t-1's barrier
      const bool dma = t + 2 < nk;
      if (dma) stage(cur == 0 ? 2 : cur - 1, kbeg + (t + 2) * SBK);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      mfma(xa, xb);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < nk) {
        // this wave's DMAs of tile t+1 have landed (t+2's stay in flight); after the barrier every wave's have
        if (dma) sat_vm_lds_barrier<G::INSTR>();
        else sat_vm_lds_barrier<0>();
        cur = cur == 2 ? 0 : cur + 1;
        frags(cur, 0, xa, xb);
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      mfma(ya, yb);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  if (a.splits > 1) {
    // ---- publish this split's partial tile; the last arriver of the tile sums all of them in split order ----
    const long tile = (long)mt * a.tiles_n + nt;
    const __amdgpu_buffer_rsrc_t rS = sat_out_rsrc(a.slab, a.slab_bytes);
    constexpr unsigned PART = (unsigned)BM * SBN * 4;   // bytes of one partial tile
    const unsigned tbase = (unsigned)(tile * a.splits) * PART;
    auto slot = [&](int i, int j) { return (unsigned)((((w * MI + i) * NJ + j) * 64 + lane) * 16); };
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) sat_st16<16>(rS, tbase + (unsigned)split * PART + slot(i, j), f4u(acc[i][j]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its write-through stores are done
    __syncthreads();
    volatile unsigned* flag = (volatile unsigned*)(smem + G::EPI_BYTES);
    if (tid == 0) {
      if constexpr (SAT_SPLIT_RELEASE) {   // agent-scope release before the ticket (second wait: Guideline 16 Pitfall 12)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      const unsigned prev = __hip_atomic_fetch_add(a.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#if SAT_SPLIT_DEBUG
      {
        const unsigned i = atomicAdd(&g_sdbg_n, 1u);
        if (i < (1u << 18)) {
          g_sdbg[4 * i] = a.dbg_launch; g_sdbg[4 * i + 1] = (unsigned)tile; g_sdbg[4 * i + 2] = (unsigned)split;
          g_sdbg[4 * i + 3] = prev;
        }
      }
#endif
      if constexpr (SAT_SPLIT_ACQUIRE) {
        if (prev == (unsigned)(a.splits - 1)) {
          // the last arriver: agent-scope acquire before it reads the other partial tiles
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      }
      *flag = prev;
    }
    __syncthreads();
    if (*flag != (unsigned)(a.splits - 1)) return;   // workgroup-uniform
    f32x4 tot[MI][NJ], part[MI][NJ];
    for (int s = 0; s < a.splits; ++s) {   // split order: the same sums whichever split arrives last
      if (s == split) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) part[i][j] = acc[i][j];
      } else {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const sat_u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(rS, (int)(tbase + (unsigned)s * PART + slot(i, j)), 0, 16);
            part[i][j] = f32x4{__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2]), __uint_as_float(u[3])};
          }
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) tot[i][j] = s == 0 ? part[i][j] : tot[i][j] + part[i][j];
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] = tot[i][j];
  }

#if SAT_SPLIT_DEBUG
  {
    unsigned x = 0;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) x ^= __float_as_uint(acc[i][j][r]) * (unsigned)(1 + ((i * NJ + j) * 4 + r));
    atomicXor(&g_sdbg_cs[(a.dbg_launch % 64) * 256 + ((long)mt * a.tiles_n + nt) % 256], x);
  }
#endif
  // ---- C: the fp32 tile through LDS, 16-B row pieces (beta = 1 adds C) ----
  sat_vm_lds_barrier<0>();   // every wave done with the ring
  float* ep = (float*)smem;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int cl = wn * G::WTN + j * 16 + fr;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) ep[(am + i * 16 + fh * 4 + r) * G::EPI_LD + cl] = acc[i][j][r];
  }
  __syncthreads();
  const int cc = tid & 15, r0 = tid >> 4;   // 16 chunks of 8 columns x 32 rows per pass
  const int col = n0 + cc * 8;
  if (col >= N) return;   // N % 8 == 0 (host-checked): a chunk is all in or all out
  const __amdgpu_buffer_rsrc_t rC = sat_out_rsrc(a.C, a.c_bytes);
#pragma unroll
  for (int it = 0; it < BM / 32; ++it) {
    const int rl = r0 + it * 32, row = m0 + rl;
    if (row >= M) break;
    float4 x0 = *(const float4*)(ep + rl * G::EPI_LD + cc * 8);
    float4 x1 = *(const float4*)(ep + rl * G::EPI_LD + cc * 8 + 4);
    const unsigned off = (unsigned)(((long)row * a.ldc + col) * 4);
    if (a.add1) {
      const float* p = a.add1 + (long)row * a.ld_add1 + col;
      x0 = f4add(x0, *(const float4*)p);
      x1 = f4add(x1, *(const float4*)(p + 4));
    }
    if (a.beta1) {
      const float* p = a.C + (long)row * a.ldc + col;
      x0 = f4add(x0, *(const float4*)p);
      x1 = f4add(x1, *(const float4*)(p + 4));
    }
    sat_st16<0>(rC, off, make_uint4(__float_as_uint(x0.x), __float_as_uint(x0.y), __float_as_uint(x0.z), __float_as_uint(x0.w)));
    sat_st16<0>(rC, off + 16, make_uint4(__float_as_uint(x1.x), __float_as_uint(x1.y), __float_as_uint(x1.z), __float_as_uint(x1.w)));
  }
}

template <int BM, bool AT, bool BT>
__global__ __launch_bounds__(512) void split_gemm_kernel(SArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[SGeom<BM>::LDS];
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  split_gemm_body<BM, AT, BT>(a, smem, blockIdx.x, gridDim.x);
  sat_stamp_end(a.st, t0);
}

// Up to kSatGemmGroupMax independent products in one grid: product i owns blocks [first[i], first[i] + blocks[i]) and
// runs the body of its own (tile height, layouts) on its own slab region and ticket range.  The table travels in the
// kernel arguments (no copy node, no memset node: a captured launch replays as it was recorded).  Products are laid
// out longest work item first, so the long items start in the first round and the short ones fill the tail; within
// a product the XCD-aware order holds as in a single launch (blocks of one residue mod 8 share an XCD whatever the
// product's first block).  No workgroup waits for another: a grid of several rounds needs no co-residency.
struct SGroupArgs {
  SArgs p[kSatGemmGroupMax];
  int first[kSatGemmGroupMax];    // first block; INT_MAX past the last product
  int blocks[kSatGemmGroupMax];
  int form[kSatGemmGroupMax];     // bit 0: B k-major, bit 1: A k-major, bit 2: 256-row tiles
  SatStamps st;
};

__global__ __launch_bounds__(512) void split_gemm_group_kernel(SGroupArgs g) {
  __shared__ __attribute__((aligned(16))) char smem[SGeom<256>::LDS];   // the taller tile's ring: one workgroup per CU
  static_assert(SGeom<256>::LDS >= SGeom<128>::LDS && SGeom<128>::LDS > 80 * 1024, "either ring keeps a CU to itself");
  const SatStampT0 t0 = sat_stamp_begin(g.st);
  const int bi = blockIdx.x;
  int idx = 0;   // wave-uniform: block index and table are scalar
#pragma unroll
  for (int i = 1; i < kSatGemmGroupMax; ++i) idx += bi >= g.first[i] ? 1 : 0;
  const SArgs& a = g.p[idx];
  const int lin = bi - g.first[idx], nwg = g.blocks[idx];
  switch (g.form[idx]) {
    case 0: split_gemm_body<128, false, false>(a, smem, lin, nwg); break;
    case 1: split_gemm_body<128, false, true>(a, smem, lin, nwg); break;
    case 2: split_gemm_body<128, true, false>(a, smem, lin, nwg); break;
    case 3: split_gemm_body<128, true, true>(a, smem, lin, nwg); break;
    case 4: split_gemm_body<256, false, false>(a, smem, lin, nwg); break;
    case 5: split_gemm_body<256, false, true>(a, smem, lin, nwg); break;
    case 6: split_gemm_body<256, true, false>(a, smem, lin, nwg); break;
    default: split_gemm_body<256, true, true>(a, smem, lin, nwg); break;
  }
  sat_stamp_end(g.st, t0);
}


struct SPlan {
  int bm = 0, splits = 1, kchunk = 0, tiles_m = 0, tiles_n = 0;
  double us = 0;
};

// Cost model (microseconds), one 8-wave workgroup per CU: a k-tile per workgroup takes what the CU's load path
// needs for its bytes (128 x 128: 32 KiB, 256 x 128: 48 KiB at ~45 GB/s per CU), the C epilogue ~1 us, and the
// last arriver of a split tile reads S-1 partial tiles at ~70 GB/s (MI355X_MICROARCH.md handoff-payload).
constexpr double kKtileUs[2] = {0.73, 1.10};   // BM = 128, 256
constexpr double kEpiUs = 1.0;
constexpr double kPartUs[2] = {0.94, 1.87};
// SatPolicy::split_gemm: 0 auto, 2 128-row tiles, 3 256-row tiles; SatPolicy::split_k > 0 forces the split count
SPlan plan_split(const SatGemm& g, bool have_ws) {
  const SatPolicy& pol = sat_policy();
  const int nk = sat_cdiv(g.K, SBK);
  SPlan best;
  best.us = 1e30;
  for (int b = 0; b < 2; ++b) {
    const int bm = b ? 256 : 128;
    if ((pol.split_gemm == 2 && bm != 128) || (pol.split_gemm == 3 && bm != 256)) continue;
    const int tm = sat_cdiv(g.M, bm), tn = sat_cdiv(g.N, SBN);
    const long tiles = (long)tm * tn;
    for (int s = 1; s <= kMaxSplits; ++s) {
      if (pol.split_k > 0 && s != pol.split_k) continue;
      if (s > 1 && (!have_ws || tiles * s > kSplitCUs || nk < 2 * s)) continue;
      const int kch = sat_cdiv(nk, s);
      const int splits = sat_cdiv(nk, kch);   // no empty split
      if (splits != s) continue;
      const double us = sat_cdiv(tiles * s, kSplitCUs) * (kch * kKtileUs[b] + kEpiUs) + (s - 1) * kPartUs[b];
      if (us < best.us - 1e-9) {
        best.bm = bm; best.splits = s; best.kchunk = kch * SBK; best.tiles_m = tm; best.tiles_n = tn; best.us = us;
      }
    }
  }
  return best;
}

// the problems this kernel takes: bf16 operands, fp32 C, C = A B (+ add1) (+ C), a k-major operand or an NN product
// the tile kernel would split with atomics, 16-B pieces
bool split_eligible(const SatGemm& g) {
  const int mode = sat_policy().split_gemm;
  if (mode == 1) return false;
  if (g.dtype != SAT_BF16 || g.c_dtype != SAT_F32 || g.batch != 1 || g.aux || g.bias || g.conv.C > 0 ||
      g.act != SAT_ACT_NONE || g.partial_splits > 1 || g.alpha != 1.f || (g.beta != 0.f && g.beta != 1.f))
    return false;
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) return false;
  // both operands k-contiguous (NN): only the products the tile kernel would split with fp32 atomics (few 128 x 128
  // tiles, K >= 1024) -- here they keep a fixed summation order (the decoder's gradients are bit-reproducible)
  if (!(g.transA || g.transB) && !((long)sat_cdiv(g.M, 128) * sat_cdiv(g.N, 128) < 160 && g.K >= 1024)) return false;
  const bool at = g.transA != 0, bt = g.transB != 0;
  if (g.lda % 8 || g.ldb % 8 || g.ldc % 4 || g.N % 8) return false;
  // a K tail (K % 8 != 0) only where the straddling 8-element chunks read zeros: an m-major A zero-padded to the next
  // multiple of 8 (SatGemm::a_tail) against a k-major B, whose rows past K the loader skips
  if (at ? (g.M % 8 && !g.a_tail) : (g.K % 8 && !(g.a_tail && bt))) return false;
  if (!bt && g.K % 8) return false;
  if (!sat_al16(g.A) || !sat_al16(g.B) || !sat_al16(g.C)) return false;
  if (g.add1 && (g.add1_dtype != SAT_F32 || !sat_al16(g.add1) || g.ld_add1 % 4)) return false;
  // buffer offsets are 32-bit: every operand and C below 2 GiB
  const long a_bytes = at ? 2L * ((long)(g.K - 1) * g.lda + (g.a_tail ? sat_cdiv(g.M, 8) * 8 : g.M))
                          : 2L * ((long)(g.M - 1) * g.lda + sat_cdiv(g.K, 8) * 8);
  const long b_bytes = bt ? 2L * ((long)(g.K - 1) * g.ldb + g.N) : 2L * ((long)(g.N - 1) * g.ldb + g.K);
  const long c_bytes = 4L * ((long)(g.M - 1) * g.ldc + g.N);
  if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31) || c_bytes >= (1L << 31)) return false;
  // auto: the long-K products (the weight gradients and the vocabulary / embedding input gradients)
  if ((mode == 0 || mode == 4) && g.K < 512) return false;   // (4: auto, without grouped launches)
  return true;
}

// ---- the joint planner of a group launch ----
// One grid of several rounds: the hardware hands blocks to CUs in block order as CUs free up, so the modelled time
// of a set is the makespan of that list schedule over kSplitCUs CUs with the single launch's measured constants per
// work item.  A split no longer has to fit one round (the last arriver of a tile never waits, so no co-residency is
// needed); what remains per split are S <= kMaxSplits, >= 2 k-tiles per split, no empty split, and the set's slab
// bytes and tickets.  Coordinate descent from (128-row tiles, unsplit): each product in turn takes the (tile
// height, split count) that shortens the whole grid most, until a sweep changes nothing.
struct GShape {
  int M, N, K, bm, splits;   // bm, splits: 0 = the planner's, else forced
};
struct GItem {
  int bm = 0, splits = 1, kchunk = 0, tiles_m = 0, tiles_n = 0, first = 0, blocks = 0;
  long slab_off = 0, slab_bytes = 0;
  int ticket_off = 0, tickets = 0, fallback = 0;
};
struct GOpt {
  int b = 0, s = 1, kch = 0, nk = 0, tm = 0, tn = 0, tickets = 0;
  long slab = 0;
  long tiles() const { return (long)tm * tn; }
  // modelled time of the work item of split j (the last split carries the K tail and, as the model's last arriver,
  // the reads of the other partials).  Charging every split item its partial store as well made the planner's sets
  // slower, alone and in the step, and was dropped.
  double item_us(int j) const {
    const int kt = kch < nk - j * kch ? kch : nk - j * kch;
    return kt * kKtileUs[b] + kEpiUs + (s > 1 && j == s - 1 ? (s - 1) * kPartUs[b] : 0.0);
  }
};

bool group_option(const GShape& sh, int b, int s, GOpt* o) {
  const int nk = sat_cdiv(sh.K, SBK), bm = b ? 256 : 128;
  if (s < 1 || s > kMaxSplits || (s > 1 && nk < 2 * s)) return false;
  const int kch = sat_cdiv(nk, s);
  if (sat_cdiv(nk, kch) != s) return false;   // no empty split
  if (s > 1 && nk - (s - 1) * kch < 2) return false;   // the last split's tail too
  o->b = b; o->s = s; o->kch = kch; o->nk = nk;
  o->tm = sat_cdiv(sh.M, bm); o->tn = sat_cdiv(sh.N, SBN);
  o->slab = s > 1 ? o->tiles() * s * bm * SBN * 4 : 0;
  o->tickets = s > 1 ? (int)o->tiles() : 0;
  return o->tiles() * s < (1L << 24);
}

// block order: products by the k-loop time of their work items, longest first (ties: the caller's order)
void group_order(const GOpt* o, const int* in, int n, int* order) {
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (in[i]) order[m++] = i;
  std::stable_sort(order, order + m,
                   [&](int x, int y) { return o[x].kch * kKtileUs[o[x].b] > o[y].kch * kKtileUs[o[y].b]; });
}

double group_model_us(const GOpt* o, const int* in, int n) {
  int order[kSatGemmGroupMax], m = 0;
  for (int i = 0; i < n; ++i) m += in[i] ? 1 : 0;
  group_order(o, in, n, order);
  std::priority_queue<double, std::vector<double>, std::greater<double>> cu;
  for (int i = 0; i < kSplitCUs; ++i) cu.push(0.0);
  double end = 0;
  for (int x = 0; x < m; ++x) {
    const GOpt& p = o[order[x]];
    for (int j = 0; j < p.s; ++j) {
      const double us = p.item_us(j);
      for (long t = 0; t < p.tiles(); ++t) {
        const double e = cu.top() + us;
        cu.pop();
        cu.push(e);
        end = e > end ? e : end;
      }
    }
  }
  return end;
}

void plan_group(const GShape* sh, int n, long slab_cap, long ticket_cap, GItem* out) {
  GOpt cur[kSatGemmGroupMax];
  int in[kSatGemmGroupMax];
  long slab = 0, tickets = 0;
  // forced split counts first (the caller's order): one the shape cannot hold, or whose region does not fit what is
  // left, falls back to a launch of its own
  for (int i = 0; i < n; ++i) {
    out[i] = GItem{};
    in[i] = 1;
    if (sh[i].splits > 0) {
      if (!group_option(sh[i], sh[i].bm == 256, sh[i].splits, &cur[i]) || slab + cur[i].slab > slab_cap ||
          tickets + cur[i].tickets > ticket_cap) {
        in[i] = 0;
        continue;
      }
      slab += cur[i].slab;
      tickets += cur[i].tickets;
    } else if (!group_option(sh[i], sh[i].bm == 256, 1, &cur[i])) {
      in[i] = 0;
    }
  }
  // with a forced split count and a free tile height, the height is chosen below at that count
  double best = group_model_us(cur, in, n);
  for (int sweep = 0; sweep < 4; ++sweep) {
    bool changed = false;
    for (int i = 0; i < n; ++i) {
      if (!in[i] || (sh[i].splits > 0 && sh[i].bm > 0)) continue;
      const GOpt keep = cur[i];
      GOpt pick = keep;
      for (int b = 0; b < 2; ++b) {
        if (sh[i].bm > 0 && (sh[i].bm == 256) != (b == 1)) continue;
        for (int s = 1; s <= kMaxSplits; ++s) {
          if (sh[i].splits > 0 && s != sh[i].splits) continue;
          GOpt o;
          if (!group_option(sh[i], b, s, &o)) continue;
          if (slab - keep.slab + o.slab > slab_cap || tickets - keep.tickets + o.tickets > ticket_cap) continue;
          cur[i] = o;
          const double us = group_model_us(cur, in, n);
          if (us < best - 1e-9) {
            best = us;
            pick = o;
          }
        }
      }
      cur[i] = pick;
      if (pick.b != keep.b || pick.s != keep.s) {
        slab += pick.slab - keep.slab;
        tickets += pick.tickets - keep.tickets;
        changed = true;
      }
    }
    if (!changed) break;
  }
  int order[kSatGemmGroupMax], m = 0;
  for (int i = 0; i < n; ++i) m += in[i] ? 1 : 0;
  group_order(cur, in, n, order);
  int first = 0;
  for (int x = 0; x < m; ++x) {
    GItem& it = out[order[x]];
    const GOpt& p = cur[order[x]];
    it.bm = p.b ? 256 : 128; it.splits = p.s; it.kchunk = p.kch * SBK; it.tiles_m = p.tm; it.tiles_n = p.tn;
    it.first = first;
    it.blocks = (int)(p.tiles() * p.s);
    first += it.blocks;
  }
  long so = 0;
  int to = 0;
  for (int i = 0; i < n; ++i) {
    if (!in[i]) {
      out[i].fallback = 1;
      continue;
    }
    out[i].slab_off = so; out[i].slab_bytes = cur[i].slab;
    out[i].ticket_off = to; out[i].tickets = cur[i].tickets;
    so += cur[i].slab;
    to += cur[i].tickets;
  }
}

// plans are pure functions of the shapes and capacities: kept, so an eager backward plans each set once
void plan_group_cached(const GShape* sh, int n, long slab_cap, long ticket_cap, GItem* out) {
  static std::mutex mu;
  static std::map<std::vector<long>, std::vector<GItem>> cache;
  std::vector<long> key{n, slab_cap, ticket_cap};
  for (int i = 0; i < n; ++i) key.insert(key.end(), {sh[i].M, sh[i].N, sh[i].K, sh[i].bm, sh[i].splits});
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it == cache.end()) {
    std::vector<GItem> v(n);
    plan_group(sh, n, slab_cap, ticket_cap, v.data());
    it = cache.emplace(key, v).first;
  }
  for (int i = 0; i < n; ++i) out[i] = it->second[i];
}

}  // namespace

size_t sat_split_gemm_ws_bytes() {
  static_assert(kSatSplitTickets >= kSplitCUs, "a split launch has at most kSplitCUs tiles");
  return (size_t)kSplitCUs * 256 * SBN * 4 + kSatSplitTickets * 4;   // partial tiles + tickets
}

// Without a workspace the kernel can only run unsplit: it takes such a call only where the planner would not split
// it anyway.  A long-K product with few tiles (the NN shapes the tile kernel splits with atomics over ~300
// workgroups, or a k-major weight gradient) falls through to sat_fast_gemm_try instead of running on a handful of
// workgroups.
static bool split_takes(const SatGemm& g) {
  if (!split_eligible(g)) return false;
  if (g.split_ws && g.split_tickets) return true;
  return plan_split(g, true).splits <= 1;
}

int sat_split_gemm_takes(const SatGemm& g) { return split_takes(g) ? 1 : 0; }

// the kernel's view of g under a plan (slab, tickets and stamps are the launch's to fill)
static SArgs split_args(const SatGemm& g, int splits, int kchunk, int tiles_m, int tiles_n) {
  const bool at = g.transA != 0, bt = g.transB != 0;
  SArgs a{};
  a.M = g.M; a.N = g.N; a.K = g.K;
  a.A = (const bf16*)g.A; a.lda = g.lda; a.B = (const bf16*)g.B; a.ldb = g.ldb;
  a.C = (float*)g.C; a.ldc = g.ldc;
  a.beta1 = g.beta != 0.f;
  a.add1 = (const float*)g.add1; a.ld_add1 = g.ld_add1;
  a.splits = splits; a.kchunk = kchunk;
  a.a_mlim = at && g.a_tail ? sat_cdiv(g.M, 8) * 8 : g.M;
  a.tiles_m = tiles_m; a.tiles_n = tiles_n;
  a.a_bytes = (unsigned)(at ? 2L * ((long)(g.K - 1) * g.lda + a.a_mlim)
                            : 2L * ((long)(g.M - 1) * g.lda + sat_cdiv(g.K, 8) * 8));
  a.b_bytes = (unsigned)(bt ? 2L * ((long)(g.K - 1) * g.ldb + g.N) : 2L * ((long)(g.N - 1) * g.ldb + g.K));
  a.c_bytes = (unsigned)(4L * ((long)(g.M - 1) * g.ldc + g.N));
  return a;
}

int sat_split_gemm_try(const SatGemm& g, hipStream_t s, int* err) {
  *err = 0;
  if (!split_takes(g)) return 0;
  const bool have_ws = g.split_ws && g.split_tickets;
  const SPlan p = plan_split(g, have_ws);
  if (p.bm == 0) return 0;
  const bool at = g.transA != 0, bt = g.transB != 0;
  SArgs a = split_args(g, p.splits, p.kchunk, p.tiles_m, p.tiles_n);
  if (p.splits > 1) {
    const long slab = (long)p.tiles_m * p.tiles_n * p.splits * p.bm * SBN * 4;
    SAT_REQUIRE(slab <= g.split_ws_bytes && (long)p.tiles_m * p.tiles_n <= kSplitCUs);
    a.slab = g.split_ws; a.slab_bytes = (unsigned)slab;
    a.tickets = g.split_tickets;
    if (!g.tickets_zeroed)
      SAT_CHECK((hipError_t)sat_zero_rows((float*)g.split_tickets, (long)p.tiles_m * p.tiles_n, 1,
                                          (long)p.tiles_m * p.tiles_n, s));
  }
  a.st = sat_launch_stamps();
#if SAT_SPLIT_DEBUG
  a.dbg_launch = ++g_sdbg_launch;
#endif
  const dim3 grid((unsigned)((long)p.tiles_m * p.tiles_n * p.splits));
  if (p.bm == 256) {
    if (at && bt) hipLaunchKernelGGL((split_gemm_kernel<256, true, true>), grid, dim3(512), 0, s, a);
    else if (at) hipLaunchKernelGGL((split_gemm_kernel<256, true, false>), grid, dim3(512), 0, s, a);
    else if (bt) hipLaunchKernelGGL((split_gemm_kernel<256, false, true>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((split_gemm_kernel<256, false, false>), grid, dim3(512), 0, s, a);
  } else {
    if (at && bt) hipLaunchKernelGGL((split_gemm_kernel<128, true, true>), grid, dim3(512), 0, s, a);
    else if (at) hipLaunchKernelGGL((split_gemm_kernel<128, true, false>), grid, dim3(512), 0, s, a);
    else if (bt) hipLaunchKernelGGL((split_gemm_kernel<128, false, true>), grid, dim3(512), 0, s, a);
    else hipLaunchKernelGGL((split_gemm_kernel<128, false, false>), grid, dim3(512), 0, s, a);
  }
  *err = (int)hipGetLastError();
  return 1;
}

static std::atomic<int64_t> g_group_launches{0};   // sat_gemm_group_launches

// SatPolicy::split_gemm = 4: the planner's choices with every product launched on its own (the A/B of the groups).
// keep_splits: every member keeps the split count of its single launch (plan_split), so its fp32 sums run over the
// same K ranges in the same order and the group writes the single launches' bits; the joint planner then chooses
// the tile heights (which do not enter the sum order: each output element adds its k-tiles in k order under either
// height), the block order and the regions.
int sat_gemm_group_launch(const SatGemm* gs, const SatPolicy* const* pol, int n, float* slab, long slab_bytes,
                          unsigned* tickets, int n_tickets, hipStream_t s, int keep_splits) {
  SAT_REQUIRE(gs && n >= 0 && n <= kSatGemmGroupMax);
  GShape sh[kSatGemmGroupMax];
  int idx[kSatGemmGroupMax], m = 0;   // members: what a launch of its own would run on the split kernel
  for (int i = 0; i < n; ++i) {
    std::optional<SatPolicyScope> scope;
    if (pol) scope.emplace(pol[i]);
    const SatPolicy& p = sat_policy();
    if (!slab || !tickets || p.split_gemm == 4 || gs[i].M <= 0 || gs[i].N <= 0 || sat_skinny_takes(gs[i]) ||
        !split_eligible(gs[i]))
      continue;
    sh[m] = GShape{gs[i].M, gs[i].N, gs[i].K, p.split_gemm == 2 ? 128 : p.split_gemm == 3 ? 256 : 0,
                   p.split_k > 0 ? p.split_k : 0};
    if (keep_splits) {
      const SPlan single = plan_split(gs[i], gs[i].split_ws && gs[i].split_tickets);
      if (single.bm == 0) continue;   // no plan under this policy: not this kernel's, as for a launch of its own
      sh[m].splits = single.splits;
    }
    idx[m++] = i;
  }
  GItem plan[kSatGemmGroupMax];
  bool grouped[kSatGemmGroupMax] = {};
  if (m >= 2) plan_group_cached(sh, m, slab_bytes, n_tickets, plan);   // a group of one is a single launch
  int members = 0;
  for (int x = 0; m >= 2 && x < m; ++x) members += plan[x].fallback ? 0 : 1;
  if (members >= 2) {
    SGroupArgs ga{};
    int total = 0;
    for (int x = 0, k = 0; x < m; ++x) {
      const GItem& it = plan[x];
      if (it.fallback) continue;
      const SatGemm& g = gs[idx[x]];
      grouped[idx[x]] = true;
      SArgs& a = ga.p[k];
      a = split_args(g, it.splits, it.kchunk, it.tiles_m, it.tiles_n);
      if (it.splits > 1) {
        SAT_REQUIRE(it.slab_off + it.slab_bytes <= slab_bytes && it.ticket_off + it.tickets <= n_tickets);
        a.slab = slab + it.slab_off / 4; a.slab_bytes = (unsigned)it.slab_bytes;
        a.tickets = tickets + it.ticket_off;
      }
#if SAT_SPLIT_DEBUG
      a.dbg_launch = ++g_sdbg_launch;
#endif
      ga.first[k] = it.first; ga.blocks[k] = it.blocks;
      ga.form[k] = (it.bm == 256 ? 4 : 0) | (g.transA ? 2 : 0) | (g.transB ? 1 : 0);
      total += it.blocks;
      ++k;
    }
    // the table in block order, so the search for a block's product is a count of first[] <= block
    for (int x = 1; x < members; ++x)
      for (int y = x; y > 0 && ga.first[y] < ga.first[y - 1]; --y) {
        std::swap(ga.p[y], ga.p[y - 1]);
        std::swap(ga.first[y], ga.first[y - 1]);
        std::swap(ga.blocks[y], ga.blocks[y - 1]);
        std::swap(ga.form[y], ga.form[y - 1]);
      }
    for (int k = members; k < kSatGemmGroupMax; ++k) ga.first[k] = INT_MAX;
    ga.st = sat_launch_stamps();
    hipLaunchKernelGGL(split_gemm_group_kernel, dim3((unsigned)total), dim3(512), 0, s, ga);
    SAT_CHECK(hipGetLastError());
    g_group_launches.fetch_add(1, std::memory_order_relaxed);
  }
  for (int i = 0; i < n; ++i) {
    if (grouped[i]) continue;
    std::optional<SatPolicyScope> scope;
    if (pol) scope.emplace(pol[i]);
    SAT_CHECK((hipError_t)sat_gemm_launch(gs[i], s));
  }
  return 0;
}

extern "C" int sat_gemm_group_plan(const SatGemmGroupShape* shapes, int n, int64_t slab_bytes, int tickets,
                                   SatGemmGroupPlan* plan) {
  SAT_REQUIRE(shapes && plan && n >= 1 && n <= kSatGemmGroupMax && slab_bytes >= 0 && tickets >= 0);
  GShape sh[kSatGemmGroupMax];
  for (int i = 0; i < n; ++i) {
    SAT_REQUIRE(shapes[i].M > 0 && shapes[i].N > 0 && shapes[i].K > 0 && shapes[i].splits >= 0 &&
                (shapes[i].tile_rows == 0 || shapes[i].tile_rows == 128 || shapes[i].tile_rows == 256));
    sh[i] = GShape{shapes[i].M, shapes[i].N, shapes[i].K, shapes[i].tile_rows, shapes[i].splits};
  }
  GItem it[kSatGemmGroupMax];
  plan_group(sh, n, slab_bytes, tickets, it);
  for (int i = 0; i < n; ++i)
    plan[i] = SatGemmGroupPlan{it[i].bm, it[i].splits, it[i].kchunk, it[i].tiles_m, it[i].tiles_n, it[i].first,
                               it[i].blocks, it[i].slab_off, it[i].slab_bytes, it[i].ticket_off, it[i].tickets,
                               it[i].fallback};
  return 0;
}

extern "C" int sat_gemm_group_block(const SatGemmGroupPlan* plan, int n, int block, int* product, int* tile_m,
                                    int* tile_n, int* split) {
  SAT_REQUIRE(plan && product && tile_m && tile_n && split && n >= 1 && n <= kSatGemmGroupMax);
  *product = -1;
  for (int i = 0; i < n; ++i)
    if (!plan[i].fallback && block >= plan[i].first_block && block < plan[i].first_block + plan[i].blocks) {
      *product = i;
      split_block_work(block - plan[i].first_block, plan[i].blocks, plan[i].tiles_m, plan[i].tiles_n, tile_m, tile_n,
                       split);
    }
  return 0;
}

size_t sat_gemm_group_slab_bound(int M, int N, int K) {
  // plan_split under any policy: S <= kMaxSplits, >= 2 k-tiles per split, and tiles x S <= kSplitCUs at its tile
  // height -- most splits with 256-row tiles, which are the fewest; the group's other tile height at the same S
  // needs no more bytes (cdiv(M, 128) x 128 <= cdiv(M, 256) x 256)
  const long tiles = (long)sat_cdiv(M, 256) * sat_cdiv(N, SBN);
  if (tiles < 1) return 0;
  long s = kSplitCUs / tiles < kMaxSplits ? kSplitCUs / tiles : kMaxSplits;
  if (s > sat_cdiv(K, SBK) / 2) s = sat_cdiv(K, SBK) / 2;
  return s > 1 ? (size_t)(tiles * s) * 256 * SBN * 4 : 0;
}

extern "C" int64_t sat_gemm_group_launches(void) { return g_group_launches.load(std::memory_order_relaxed); }

extern "C" size_t sat_gemm_group_workspace_bytes(void) {
  return sat_split_gemm_ws_bytes() - kSatSplitTickets * 4 + (size_t)kSatGroupTickets * 4;
}

#if SAT_SPLIT_DEBUG
// diagnostics builds: copy the ticket-draw records {launch, tile, split, prev} (n4 = 4 x records) and reset them
extern "C" int sat_split_debug_read(unsigned* out, int n4, unsigned* count) {
  SAT_CHECK(hipDeviceSynchronize());
  SAT_CHECK(hipMemcpyFromSymbol(count, HIP_SYMBOL(g_sdbg_n), sizeof(unsigned)));
  const unsigned m = *count * 4 < (unsigned)n4 ? *count * 4 : (unsigned)n4;
  if (m) SAT_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sdbg), m * sizeof(unsigned)));
  const unsigned z = 0;
  SAT_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_sdbg_n), &z, sizeof(unsigned)));
  return 0;
}
extern "C" int sat_split_debug_checksums(unsigned* out) {   // 64 x 256 words, then zeroed
  SAT_CHECK(hipDeviceSynchronize());
  SAT_CHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sdbg_cs), 64 * 256 * sizeof(unsigned)));
  static unsigned zeros[64 * 256] = {};
  SAT_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_sdbg_cs), zeros, sizeof(zeros)));
  return 0;
}
#endif

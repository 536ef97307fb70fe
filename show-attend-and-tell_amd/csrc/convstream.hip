// Weight-stationary streaming kernel for short-K 1x1 convolutions (gfx950 / MI355X).
//
//   C[M,N] = act(A[M,K] . B[N,K]^T + bias[N] (+ res[M,N]))       bf16 in/out, fp32 accumulate
//   A row m = the NHWC input pixel of output pixel m (stride 1: row m; stride s: (n, oh*s, ow*s)),
//   K = Cin in {64, 128, 256, 512}, B = conv weights [Cout][Cin].  (K = 1024 with 128 VGPRs of B per
//   lane measured slower than convpipe.hip on L3 c1: 27.1 vs 23 us, profiles/r2_s10_stream_k1024.txt.)
//
// These are the ResNet152 bottleneck c3 (+ identity / projection residual) and downsample convs
// and the K <= 512 c1 convs: 2-13 GFLOP each against 60-460 MB of activations, so they are
// bound by HBM (output + residual + input bytes), not by MFMA.  The 128-row tile kernel
// (convgemm.hip) pays, per 128 x 128 tile, a full A + B staging round trip, a K-loop of 1-8
// k-tiles, and an epilogue that nothing overlaps; at K = 256 that ran at 2.9 TB/s (L3 c3).
// Here instead:
//   * one persistent workgroup per CU (8 waves) owns a 128-column slice of N; each wave holds its
//     16 columns of B for ALL of K in registers (loaded once: K/32 x 16 B per lane), so the only
//     operand streamed per item is an MT x K tile of A (LDS-DMA, double-buffered);
//   * the workgroup walks M-tiles (items) of its slice; the 8 slices of one M-tile sequence are
//     placed on one XCD (blocks b, b+8, ... share an L2), so each A tile is fetched from HBM once
//     and re-served from L2 to the other slices;
//   * C^T = B . A^T on v_mfma_f32_16x16x32_bf16 (B fragments as the first operand): a lane then
//     holds 4 consecutive output COLUMNS of one row, so the epilogue (bias, fp32 residual add,
//     activation, one bf16 rounding -- the same arithmetic as the other conv kernels) needs no
//     LDS transpose: 8-byte residual loads and 8-byte stores, 32 contiguous bytes per row per wave;
//   * pipeline per item: barrier -> LDS-DMA of item i+2's A tile and residual tile into the free
//     stage of a 3-stage ring (item i+1 is landing) -> fragment reads + MFMAs -> epilogue (residual
//     from LDS) -> 8-B stores, with a counted vmcnt (never 0 in the loop) so the next item's DMAs
//     and the last two items' stores stay in flight across the barrier; every global read in the
//     loop is a DMA, so the compiler inserts no vmcnt waits of its own;
//   * LDS image lane-linear (DMA), swizzle on the source: 16-B chunk c of row r at slot
//     c ^ (r & 15) (rows >= 256 B) or c ^ ((r >> 1) & 7) (128-B rows) -> conflict-free
//     ds_read_b128 fragment reads (verified for every lane group).
//   * chained form (conv1x1_chain_kernel, sat_conv1x1_chain): one slice of whole rows; after the epilogue barrier
//     the finished output tile is the A operand of the NEXT bottleneck's c1 (weights register-stationary like B),
//     computed beside the whole-row stores, so the c3's output is not read back for it: (K, N -> N2) = (64, 256 -> 64),
//     (64, 256 -> 128), (128, 512 -> 128), both outputs bit-identical to the two launches.
//   * projection form (conv1x1_proj_kernel, sat_conv1x1_proj): the c3 of a stage's first bottleneck, whose residual is
//     the downsample conv of the block input.  The wave also keeps its columns of the downsample weights in registers,
//     the stage holds the block input's tile (MT x Kp, strided source for layer2) in place of the residual tile, and
//     the residual bf16(accP + biasP) is formed in registers -- the downsample launch's arithmetic -- so its output is
//     neither written nor read: (K, N, Kp, stride) = (64, 256, 64, 1) plain and chained, (128, 512, 256, 2) plain,
//     bit-identical to the separate launches.
#include "sat_common.h"

#ifndef SAT_STREAM_WT_BYTES
#define SAT_STREAM_WT_BYTES (64L << 20)
#endif

#include "sat_internal.h"
#include "sat_lds_pipe.h"

namespace {

constexpr int S_NW = 8, S_BN = 16 * S_NW;    // 8 waves x 16 columns

struct SArgs {
  int M, N, K;
  const bf16* A; const bf16* B; bf16* C;
  const float* bias;
  const bf16* res;
  int H, W, Cin, stride, OH, OW;     // input geometry (1x1 conv, pad 0)
  int slices, per_slice, items;      // N / 128, workgroups per slice, M-tiles
  int xcd_group;                     // 1: slice = (b / 8) % slices (one M-tile sequence per XCD)
  int wt;                            // write-through output stores (sat_common.h), else write-back
  unsigned a_bytes;
  // chained form: the next bottleneck's c1, C2[M, N2] = relu(C . B2[N2, N]^T + bias2), computed from the finished
  // output tile while it is still in LDS (N2 is a template parameter)
  const bf16* B2; const float* bias2; bf16* C2;
  int wt2;                           // write-through stores of C2
  // projection mode: the residual is the block's downsample conv, res[M, N] = bf16(P . BP[N, KP]^T + biasP), formed in
  // registers from the block input's tile (P: NHWC [*, pH, pW, KP], pixel (n, oh * pstride, ow * pstride) for row m)
  const bf16* P; const bf16* BP; const float* biasP;
  int pH, pW, pstride, pOH, pOW;
  unsigned p_bytes;
  SatStamps st;                      // in-kernel launch timestamps (SatPolicy::stamps)
};

// sat_vm_lds_barrier for a workgroup-uniform runtime n (the literal comes from a switch)
__device__ __forceinline__ void s_wait_barrier(int n) {
  switch (n) {
#define SW_CASE(k) case k: sat_vm_lds_barrier<k>(); break;
    SW_CASE(1) SW_CASE(2) SW_CASE(3) SW_CASE(4) SW_CASE(5) SW_CASE(6) SW_CASE(7) SW_CASE(8) SW_CASE(9) SW_CASE(10)
    SW_CASE(11) SW_CASE(12) SW_CASE(13) SW_CASE(14) SW_CASE(15) SW_CASE(16) SW_CASE(17) SW_CASE(18) SW_CASE(19)
    SW_CASE(20) SW_CASE(21) SW_CASE(22) SW_CASE(23) SW_CASE(24)
#undef SW_CASE
    default: sat_vm_lds_barrier<0>(); break;
  }
}

// KT = K / 32 k-steps, MB = 16-row m-blocks per item (MT = 16 * MB rows), NB = 16-column n-blocks
// per wave (the workgroup's slice is 128 * NB columns), N2B = 16-column n-blocks of the chained c1's output
// (0: no chain; 4 or 8: the slice is the whole row, N = 128 * NB, and is the chained product's K), KTP = KP / 32
// k-steps of the projected residual (0: none; the residual is then RES's tensor), PSTR: its input is strided
template <int KT, int MB, int NB, bool RES, int ACT, bool STRIDED, int N2B = 0, int KTP = 0, bool PSTR = false>
__device__ __forceinline__ void conv1x1_stream_kernel_body(const SArgs& a) {
  constexpr int K = KT * 32, MT = MB * 16, ROWB = K * 2;
  constexpr bool PROJ = KTP > 0;
  static_assert(!(PROJ && RES), "the projected residual replaces the residual tensor");
  constexpr int KP = KTP * 32, PROWB = PROJ ? KP * 2 : 128;   // block-input row bytes
  constexpr int PTILE = PROJ ? MT * PROWB : 0;               // block-input tile bytes, behind the R/O tile
  constexpr int SN = S_BN * NB, RROWB = SN * 2;            // slice columns, residual row bytes
  constexpr int TILE = MT * ROWB;                           // A tile bytes
  constexpr int RTILE = MT * RROWB;                          // residual-in / output-out tile bytes
  constexpr int STG = TILE + RTILE + PTILE;                 // one LDS stage
  constexpr int NSTG = 3;                                   // items i, i+1 (landing), i+2 (issued)
  static_assert(NSTG * STG <= 160 * 1024, "the ring must fit in LDS");
  constexpr int DMA_A = TILE / (S_NW * 64 * 16);            // 16-B DMAs per lane per item
  constexpr int DMA_R = RTILE / (S_NW * 64 * 16);
  static_assert(DMA_A * S_NW * 64 * 16 == TILE && DMA_R * S_NW * 64 * 16 == RTILE, "whole 8 KiB rounds");
  constexpr int ST = RTILE / (S_NW * 64 * 16);              // 16-B row-segment stores per lane per item
  constexpr int DMA_P = PTILE / (S_NW * 64 * 16);
  static_assert(DMA_P * S_NW * 64 * 16 == PTILE, "whole 8 KiB rounds");
  constexpr int DMA_N = DMA_A + (RES ? DMA_R : 0) + DMA_P;
  constexpr int CPR = RROWB / 16;                           // 16-B chunks per output row
  // chained c1: wave w computes n-block w of all MB m-blocks (N2 = 128) or n-block w % 4 of m-half w / 4 (N2 = 64);
  // the output tile leaves as whole rows through LDS where it fits, else m-blocks in pairs as 16-B stores
  constexpr int N2 = 16 * N2B, KT2 = SN / 32, MB2 = N2B == 4 ? MB / 2 : MB;
  constexpr bool X1_LDS = N2B && MT * N2 * 2 <= TILE;       // the chained output tile is staged in the A tile's LDS
  constexpr int ST2 = N2B ? (X1_LDS ? 1 : MB2 / 2) : 0;     // 16-B chained-output stores per lane per item
  static_assert(N2B == 0 || ((N2B == 4 || N2B == 8) && MB2 % 2 == 0), "chained c1: 64 or 128 columns, m-block pairs");
  static_assert(DMA_N + 2 * (ST + ST2) <= 24, "s_wait_barrier's counted cases");
  __shared__ __attribute__((aligned(16))) char smem[NSTG * STG];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  int slice, grp;
  if (a.xcd_group) {
    slice = (b / 8) % a.slices;
    grp = (b % 8) + 8 * (b / (8 * a.slices));
  } else {
    slice = b % a.slices;
    grp = b / a.slices;
  }
  const int ns = slice * SN;                 // the workgroup's columns
  const int wc = w * 16 * NB;                // this wave's first column within the slice
  const int fr = lane & 15, fh = lane >> 4;

  // B fragments for all of K (registers for the whole kernel): lane (fh, fr) of n-block nb holds
  // B[ns + wc + nb*16 + fr][32 ks + 8 fh ..]
  bf16x8 bq[KT][NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const bf16* bp = a.B + (long)(ns + wc + nb * 16 + fr) * K + 8 * fh;
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) bq[ks][nb] = *(const bf16x8*)(bp + 32 * ks);
  }
  float bias4[NB][4];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 4; ++j) bias4[nb][j] = a.bias ? a.bias[ns + wc + nb * 16 + 4 * fh + j] : 0.f;
  // projected residual: this wave's columns of BP for all of KP and their bias, registers like bq / bias4
  bf16x8 pq[PROJ ? KTP : 1][NB];
  float biasp4[NB][4];
  if constexpr (PROJ) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const bf16* bp = a.BP + (long)(ns + wc + nb * 16 + fr) * KP + 8 * fh;
#pragma unroll
      for (int ks = 0; ks < KTP; ++ks) pq[ks][nb] = *(const bf16x8*)(bp + 32 * ks);
#pragma unroll
      for (int j = 0; j < 4; ++j) biasp4[nb][j] = a.biasP ? a.biasP[ns + wc + nb * 16 + 4 * fh + j] : 0.f;
    }
  }
  // chained c1: this wave's 16 rows of B2 for all of its K (= N), registers for the whole kernel like bq
  const int nb2 = N2B == 4 ? (w & 3) : w, mb2 = N2B == 4 ? (w >> 2) * MB2 : 0;
  bf16x8 wq[KT2 > 0 && N2B ? KT2 : 1];
  float bias2[4];
  if constexpr (N2B > 0) {
    const bf16* wp = a.B2 + (long)(nb2 * 16 + fr) * SN + 8 * fh;
#pragma unroll
    for (int ks = 0; ks < KT2; ++ks) wq[ks] = *(const bf16x8*)(wp + 32 * ks);
#pragma unroll
    for (int j = 0; j < 4; ++j) bias2[j] = a.bias2 ? a.bias2[nb2 * 16 + 4 * fh + j] : 0.f;
    // consume every register-stationary operand here: otherwise the compiler's vmcnt tracking still sees the
    // loads pending inside the item loop and inserts waits that also drain the next items' DMAs and the stores
#pragma unroll
    for (int ks = 0; ks < KT2; ++ks) asm volatile("" ::"v"(wq[ks]));
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(bias2[j]));
  }
  if constexpr (N2B > 0 || PROJ) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int ks = 0; ks < KT; ++ks) asm volatile("" ::"v"(bq[ks][nb]));
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(bias4[nb][j]));
    }
  }
  if constexpr (PROJ) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int ks = 0; ks < KTP; ++ks) asm volatile("" ::"v"(pq[ks][nb]));
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(biasp4[nb][j]));
    }
  }

  const unsigned c_bytes = (unsigned)((long)a.M * a.N * 2);
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)a.A, (short)0, (int)a.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)a.C, (short)0, (int)c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rR =
      __builtin_amdgcn_make_buffer_rsrc((void*)(RES ? a.res : a.C), (short)0, (int)c_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rC2 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(N2B ? a.C2 : a.C), (short)0, (int)(N2B ? (unsigned)((long)a.M * N2 * 2) : c_bytes), 0x00020000);
  const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(PROJ ? a.P : a.A), (short)0, (int)(PROJ ? a.p_bytes : a.a_bytes), 0x00020000);

  // Every global read of the loop is an LDS-DMA (A tile and residual tile of the next item), so the
  // only vmcnt waits are the counted ones below; rows >= M read zeros through out-of-range buffer
  // offsets and their stores are dropped the same way, so every lane issues every instruction.
  auto stage = [&](int it, int buf) {
    const int m0 = it * MT;
    char* st = smem + buf * STG;
#pragma unroll
    for (int d = 0; d < DMA_A; ++d) {
      const int byte = (d * S_NW + w) * 1024 + lane * 16;   // LDS offset of this lane's 16 B
      const int r = byte / ROWB, pc = (byte % ROWB) / 16;
      int c;
      if constexpr (ROWB >= 256) c = (pc & ~15) | ((pc & 15) ^ (r & 15));
      else c = pc ^ ((r >> 1) & 7);
      const int m = m0 + r;
      unsigned off = kSatOOB;
      if (m < a.M) {
        long pix = m;
        if constexpr (STRIDED) {
          const int ohw = a.OH * a.OW;
          const int n = m / ohw, rem = m - n * ohw;
          const int oh = rem / a.OW, ow = rem - oh * a.OW;
          pix = ((long)n * a.H + oh * a.stride) * a.W + ow * a.stride;
        }
        off = (unsigned)((pix * K + 8 * c) * 2);
      }
      sat_bdma16(rA, st + (d * S_NW + w) * 1024, off);
    }
    if constexpr (RES) {   // residual rows of this slice's columns, 16-B chunk c at slot c ^ (r & 15) in 256-B groups
#pragma unroll
      for (int d = 0; d < DMA_R; ++d) {
        const int byte = (d * S_NW + w) * 1024 + lane * 16;
        const int r = byte / RROWB, pc = (byte % RROWB) / 16, c = (pc & ~15) | ((pc & 15) ^ (r & 15));
        const int m = m0 + r;
        const unsigned off = m < a.M ? (unsigned)(((long)m * a.N + ns + 8 * c) * 2) : kSatOOB;
        sat_bdma16(rR, st + TILE + (d * S_NW + w) * 1024, off);
      }
    }
    if constexpr (PROJ) {   // the block input's rows of this item, the A tile's swizzle at its own row length
#pragma unroll
      for (int d = 0; d < DMA_P; ++d) {
        const int byte = (d * S_NW + w) * 1024 + lane * 16;
        const int r = byte / PROWB, pc = (byte % PROWB) / 16;
        int c;
        if constexpr (PROWB >= 256) c = (pc & ~15) | ((pc & 15) ^ (r & 15));
        else c = pc ^ ((r >> 1) & 7);
        const int m = m0 + r;
        unsigned off = kSatOOB;
        if (m < a.M) {
          long pix = m;
          if constexpr (PSTR) {
            const int ohw = a.pOH * a.pOW;
            const int n = m / ohw, rem = m - n * ohw;
            const int oh = rem / a.pOW, ow = rem - oh * a.pOW;
            pix = ((long)n * a.pH + oh * a.pstride) * a.pW + ow * a.pstride;
          }
          off = (unsigned)((pix * KP + 8 * c) * 2);
        }
        sat_bdma16(rP, st + TILE + RTILE + (d * S_NW + w) * 1024, off);
      }
    }
  };

  // A fragment: row mb*16 + fr, logical chunk 4 ks + fh
  auto afrag = [&](const char* base, int mb, int ks) {
    const int r = mb * 16 + fr, c = ks * 4 + fh;
    int pc;
    if constexpr (ROWB >= 256) pc = (c & ~15) | ((c & 15) ^ (r & 15));
    else pc = c ^ ((r >> 1) & 7);
    return *(const bf16x8*)(base + r * ROWB + 16 * pc);
  };
  // block-input fragment: row mb*16 + fr, logical chunk 4 ks + fh of the P tile
  auto pfrag = [&](const char* pbase, int mb, int ks) {
    const int r = mb * 16 + fr, c = ks * 4 + fh;
    int pc;
    if constexpr (PROWB >= 256) pc = (c & ~15) | ((c & 15) ^ (r & 15));
    else pc = c ^ ((r >> 1) & 7);
    return *(const bf16x8*)(pbase + r * PROWB + 16 * pc);
  };

  int it = grp;
  if (it >= a.items) return;   // workgroup-uniform: no barrier is reached by part of a group
  const int step = a.per_slice;
  stage(it, 0);
  if (it + step < a.items) stage(it + step, 1);
  int buf = 0;
  for (int k = 0;; ++k) {
    const int nxt2 = it + 2 * step;
    // wait for this wave's DMAs of item `it`; younger: the next item's DMAs (if any) and the
    // stores of the previous one or two items -- they stay in flight across the barrier.  After it
    // every wave's DMAs of `it` have landed and every wave finished reading stage (k+2) % 3.
    const int younger = (it + step < a.items ? DMA_N : 0) + (k >= 1 ? ST + ST2 : 0) + (k >= 2 ? ST + ST2 : 0);
    s_wait_barrier(younger);
    if (nxt2 < a.items) stage(nxt2, buf == 0 ? 2 : buf - 1);
    __builtin_amdgcn_sched_barrier(0);
    const char* base = smem + buf * STG;
    // projected residual first: the downsample conv's arithmetic (k-steps ascending, one accumulator per output,
    // bias, one bf16 rounding), kept packed -- 2 registers per 4 outputs -- until the epilogue adds it
    sat_u32x2 rproj[PROJ ? MB : 1][NB];
    if constexpr (PROJ) {
      const char* pbase = base + TILE + RTILE;
      f32x4 accp[MB][NB];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) accp[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KTP; ++ks) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const bf16x8 pf = pfrag(pbase, mb, ks);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            accp[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pq[ks][nb], pf, accp[mb][nb], 0, 0, 0);
        }
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          sat_u32x2 t;
          bf16* tb = (bf16*)&t;
#pragma unroll
          for (int j = 0; j < 4; ++j) tb[j] = (bf16)apply_act(accp[mb][nb][j] + biasp4[nb][j], SAT_ACT_NONE);
          rproj[mb][nb] = t;
        }
    }
    f32x4 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 af[2][MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) af[0][mb] = afrag(base, mb, 0);
#pragma unroll
    for (int ks = 0; ks < KT; ++ks) {
      if (ks + 1 < KT) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) af[(ks + 1) & 1][mb] = afrag(base, mb, ks + 1);
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[ks][nb], af[ks & 1][mb], acc[mb][nb], 0, 0, 0);
    }
    // epilogue: lane holds C[m0 + mb*16 + fr][ns + wc + nb*16 + 4 fh + j], j = 0..3.  bias, the residual
    // (from the stage's R/O tile), activation, one bf16 rounding; the 8 result bytes go back to the
    // same R/O slot they came from, and after a workgroup barrier the tile leaves as whole rows
    // (16 B per lane, 256 / 512 contiguous bytes per row) instead of 8-B pieces of 16 rows.
    char* ro = (char*)base + TILE;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int r = mb * 16 + fr;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int lc = (wc + nb * 16 + 4 * fh) / 8;                     // logical 16-B chunk of these 8 B
        const int pc = (lc & ~15) | ((lc & 15) ^ (r & 15));
        sat_u32x2* slot = (sat_u32x2*)(ro + r * RROWB + 16 * pc + 8 * (fh & 1));
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[mb][nb][j] + bias4[nb][j];
        if constexpr (RES) {
          const sat_u32x2 rv = *slot;
          const bf16* h = (const bf16*)&rv;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += (float)h[j];
        }
        if constexpr (PROJ) {
          const bf16* h = (const bf16*)&rproj[mb][nb];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += (float)h[j];
        }
        sat_u32x2 o;
        bf16* ob = (bf16*)&o;
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[j] = (bf16)apply_act(v[j], ACT);
        *slot = o;
      }
    }
    sat_lds_barrier();   // LDS only: DMAs and stores stay in flight
    // the row reads are asm statements with their own lgkmcnt wait: ahead of an LDS read it can see, the compiler
    // waits for the LDS-DMAs in flight with a vmcnt(0) of its own, which drained the next items' DMAs and the last
    // items' stores in every iteration (the barrier above already orders these reads after the epilogue's writes)
    sat_u32x4 rows[ST];
#pragma unroll
    for (int p = 0; p < ST; ++p) {
      const int t = p * S_NW * 64 + tid, r = t / CPR, lc = t % CPR;
      const int pc = (lc & ~15) | ((lc & 15) ^ (r & 15));
      asm volatile("ds_read_b128 %0, %1" : "=v"(rows[p]) : "v"((unsigned)(uintptr_t)(sat_lds_char*)(ro + r * RROWB + 16 * pc)) : "memory");
    }
    static_assert(ST == 1 || ST == 2 || ST == 4, "the wait below names every row register");
    if constexpr (ST == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rows[0]), "+v"(rows[1]), "+v"(rows[2]), "+v"(rows[3]) :: "memory");
    else if constexpr (ST == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rows[0]), "+v"(rows[1]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rows[0]) :: "memory");
#pragma unroll
    for (int p = 0; p < ST; ++p) {
      const int t = p * S_NW * 64 + tid, r = t / CPR, lc = t % CPR;
      const sat_u32x4 u = rows[p];
      const int m = it * MT + r;
      const unsigned off = m < a.M ? (unsigned)(((long)m * a.N + ns + 8 * lc) * 2) : kSatOOB;
      if (a.wt) __builtin_amdgcn_raw_buffer_store_b128(u, rC, (int)off, 0, SAT_OUT_CPOL);
      else __builtin_amdgcn_raw_buffer_store_b128(u, rC, (int)off, 0, 0);
    }
    if constexpr (N2B > 0) {
      // chained c1 on the finished tile (bias, residual, activation applied, rounded once to bf16): A fragments are
      // row mb*16 + fr, logical chunk 4 ks + fh of the R/O tile -- the A tile's read pattern and swizzle; the stage is
      // refilled only after the next iteration's barrier.  k-steps ascending, one accumulator per output: the
      // arithmetic of the standalone c1 launch.
      f32x4 acc2[MB2];
#pragma unroll
      for (int i = 0; i < MB2; ++i) acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KT2; ++ks) {
#pragma unroll
        for (int i = 0; i < MB2; ++i) {
          const int r = (mb2 + i) * 16 + fr, c = ks * 4 + fh;
          const int pc = (c & ~15) | ((c & 15) ^ (r & 15));
          const bf16x8 xf = *(const bf16x8*)(ro + r * RROWB + 16 * pc);
          acc2[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[ks], xf, acc2[i], 0, 0, 0);
        }
      }
      // lane holds C2[m0 + (mb2 + i)*16 + fr][nb2*16 + 4 fh + j], j = 0..3: bias, ReLU, one bf16 rounding
      sat_u32x2 o[MB2];
#pragma unroll
      for (int i = 0; i < MB2; ++i) {
        sat_u32x2 t;
        bf16* ob = (bf16*)&t;
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[j] = (bf16)apply_act(acc2[i][j] + bias2[j], SAT_ACT_RELU);
        o[i] = t;
      }
      if constexpr (X1_LDS) {
        // the C2 tile fits the stage's A tile (every wave read its A fragments before the barrier above, and the
        // stage is refilled after the next one): the 8-B pieces go there, 16-B chunk c of row r at slot
        // c ^ (r % chunks per row), and after a barrier the tile leaves as whole rows, 16 B per lane -- a
        // write-through store of part of a row is a fabric write of its own
        constexpr int CPR2 = N2 * 2 / 16;
        static_assert(MT * N2 * 2 == S_NW * 64 * 16, "one 16-B row segment per lane");
        char* xt = (char*)base;
#pragma unroll
        for (int i = 0; i < MB2; ++i) {
          const int r = (mb2 + i) * 16 + fr, lc = (nb2 * 16 + 4 * fh) / 8;
          *(sat_u32x2*)(xt + r * (N2 * 2) + 16 * (lc ^ (r & (CPR2 - 1))) + 8 * (fh & 1)) = o[i];
        }
        sat_lds_barrier();
        const int r = tid / CPR2, lc = tid % CPR2;
        sat_u32x4 u;   // asm, as the row reads above
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(u) : "v"((unsigned)(uintptr_t)(sat_lds_char*)(xt + r * (N2 * 2) + 16 * (lc ^ (r & (CPR2 - 1))))) : "memory");
        const int m = it * MT + r;
        const unsigned off = m < a.M ? (unsigned)(((long)m * N2 + 8 * lc) * 2) : kSatOOB;
        if (a.wt2) __builtin_amdgcn_raw_buffer_store_b128(u, rC2, (int)off, 0, SAT_OUT_CPOL);
        else __builtin_amdgcn_raw_buffer_store_b128(u, rC2, (int)off, 0, 0);
      } else {
        // a larger C2 tile leaves from the registers.  Lanes fh and fh ^ 1 swap halves of an m-block pair: the even
        // lane stores columns 4 fh .. 4 fh + 7 of m-block i, the odd one 4 (fh - 1) .. 4 fh + 3 of m-block i + 1 --
        // whole 16-B stores; rows >= M are dropped through the out-of-range offset, so every lane issues every
        // store (the counted vmcnt)
        const bool odd = fh & 1;
#pragma unroll
        for (int i = 0; i < MB2; i += 2) {
          const sat_u32x2 send = odd ? o[i] : o[i + 1];
          const unsigned gx = (unsigned)__shfl_xor((int)send.x, 16, 64), gy = (unsigned)__shfl_xor((int)send.y, 16, 64);
          const sat_u32x4 u = odd ? sat_u32x4{gx, gy, o[i + 1].x, o[i + 1].y} : sat_u32x4{o[i].x, o[i].y, gx, gy};
          const int m = it * MT + (mb2 + i + (odd ? 1 : 0)) * 16 + fr;
          const int col = nb2 * 16 + 4 * fh - (odd ? 4 : 0);
          const unsigned off = m < a.M ? (unsigned)(((long)m * N2 + col) * 2) : kSatOOB;
          if (a.wt2) __builtin_amdgcn_raw_buffer_store_b128(u, rC2, (int)off, 0, SAT_OUT_CPOL);
          else __builtin_amdgcn_raw_buffer_store_b128(u, rC2, (int)off, 0, 0);
        }
      }
    }
    it += step;
    if (it >= a.items) break;
    buf = buf == 2 ? 0 : buf + 1;
  }
}

template <int KT, int MB, int NB, bool RES, int ACT, bool STRIDED>
__global__ __launch_bounds__(S_NW * 64) void conv1x1_stream_kernel(SArgs a) {
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  conv1x1_stream_kernel_body<KT, MB, NB, RES, ACT, STRIDED>(a);
  sat_stamp_end(a.st, t0);
}

// the chained form (bottleneck c3 + residual + ReLU, then the next bottleneck's c1 + ReLU): one 128 * NB column
// slice = whole output rows
template <int KT, int MB, int NB, int N2B>
__global__ __launch_bounds__(S_NW * 64) void conv1x1_chain_kernel(SArgs a) {
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  conv1x1_stream_kernel_body<KT, MB, NB, true, SAT_ACT_RELU, false, N2B>(a);
  sat_stamp_end(a.st, t0);
}

// the projection forms (a stage's first bottleneck: c3 + ReLU with the downsample conv of the block input as the
// residual, computed in registers), plain (N2B = 0) or chained
template <int KT, int MB, int NB, int N2B, int KTP, bool PSTR>
__global__ __launch_bounds__(S_NW * 64) void conv1x1_proj_kernel(SArgs a) {
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  conv1x1_stream_kernel_body<KT, MB, NB, false, SAT_ACT_RELU, false, N2B, KTP, PSTR>(a);
  sat_stamp_end(a.st, t0);
}

// CUs the persistent grids are sized for (0: the query failed)
int stream_cus() {
#ifdef SAT_STREAM_CUS   // diagnostics builds: this many CUs (the rest left to a concurrent decoder)
  return sat_cu_count() > 0 ? SAT_STREAM_CUS : 0;
#else
  return sat_cu_count();
#endif
}

template <int KT, int MB, int NB, bool RES, bool STRIDED>
void launch_s(int act, dim3 grid, hipStream_t s, const SArgs& a) {
  if (act == SAT_ACT_RELU)
    hipLaunchKernelGGL((conv1x1_stream_kernel<KT, MB, NB, RES, SAT_ACT_RELU, STRIDED>), grid, dim3(S_NW * 64), 0, s, a);
  else
    hipLaunchKernelGGL((conv1x1_stream_kernel<KT, MB, NB, RES, SAT_ACT_NONE, STRIDED>), grid, dim3(S_NW * 64), 0, s, a);
}
template <int KT, int MB, int NB>
void launch_kt(bool res, bool strided, int act, dim3 grid, hipStream_t s, const SArgs& a) {
  if (res) {
    if (strided) launch_s<KT, MB, NB, true, true>(act, grid, s, a);
    else launch_s<KT, MB, NB, true, false>(act, grid, s, a);
  } else {
    if (strided) launch_s<KT, MB, NB, false, true>(act, grid, s, a);
    else launch_s<KT, MB, NB, false, false>(act, grid, s, a);
  }
}

}  // namespace

// Returns 1 if the 1x1 conv was launched by the streaming kernel (error code in *err), 0 otherwise.
int sat_conv_stream_try(const SatGemm& g, hipStream_t s, int* err) {
  *err = 0;
  const int mode = sat_policy().conv_stream;   // 0 auto, 1 off, 2 every eligible problem
  if (mode == 1) return 0;
  const SatConvGeom& cv = g.conv;
  if (cv.C <= 0 || cv.KH != 1 || cv.KW != 1 || cv.pad != 0) return 0;
  if (g.dtype != SAT_BF16 || g.c_dtype != SAT_BF16 || g.batch != 1 || g.aux || g.transB) return 0;
  if (g.beta != 0.f || g.alpha != 1.f || g.partial_splits > 1) return 0;
  if (g.act != SAT_ACT_NONE && g.act != SAT_ACT_RELU) return 0;
  const int K = g.K;
  if (!(K == 64 || K == 128 || K == 256 || K == 512) || g.ldb != K) return 0;
  if (g.N % S_BN || g.ldc != g.N) return 0;
  if (g.add1 && (g.add1_dtype != SAT_BF16 || g.ld_add1 != g.N || !sat_al16(g.add1))) return 0;
  if (!sat_al16(g.A) || !sat_al16(g.B) || !sat_al16(g.C) || (g.bias && ((uintptr_t)g.bias & 15))) return 0;
  const long a_bytes = 2L * cv.N * cv.H * cv.W * cv.C;
  if (a_bytes >= (1L << 31) || (long)g.M * g.N >= (1L << 31)) return 0;
  const bool strided = cv.stride != 1 || cv.OH != cv.H || cv.OW != cv.W;
  const int cus = stream_cus();
  if (cus == 0) return 0;
  // NB = 2 (256-column slices; each A fragment read feeds two MFMAs) when N allows it, 32-row items;
  // NB = 1 (128-column slices) otherwise, 64-row items (32 at K = 512)
  const int NB = g.N % (2 * S_BN) == 0 ? 2 : 1;
#ifndef SAT_STREAM_MB256   // diagnostics builds: 16-row blocks per item at K = 256 with 256-column slices
#define SAT_STREAM_MB256 2
#endif
  const int MB = NB == 2 ? (K == 64 ? 4 : K == 256 ? SAT_STREAM_MB256 : 2) : (K >= 512 ? 2 : 4);
  const int MT = MB * 16;
  const int slices = g.N / (S_BN * NB);
  const int items = sat_cdiv(g.M, MT);
  if (mode == 0) {
    // HBM-bound shapes only: enough items per workgroup to pipeline (>= ~3)
    if ((long)items * slices < 2L * cus) return 0;
  }
  // K = 64 with 128-column slices: two workgroups per CU fit (3 x 24 KiB of LDS, <= 128 VGPRs each)
  // and hide each other's barrier / epilogue latency; the other rings take 72-144 KiB: one per CU
  const int wpc = (K <= 64 && NB == 1) ? 2 : 1;
  int per_slice = cus * wpc / slices;
  if (per_slice < 1) per_slice = 1;
  if (per_slice > items) per_slice = items;
  SArgs a{};
  a.M = g.M; a.N = g.N; a.K = K;
  a.A = (const bf16*)g.A; a.B = (const bf16*)g.B; a.C = (bf16*)g.C;
  // write-through only for outputs up to SAT_STREAM_WT_BYTES (layer3 / layer4 sizes); the layer1 / layer2 outputs
  // (100-200 MB, HBM-bound kernels) keep write-back stores
  a.wt = 2L * g.M * g.N <= (long)SAT_STREAM_WT_BYTES;
  a.bias = g.bias; a.res = (const bf16*)g.add1;
  a.H = cv.H; a.W = cv.W; a.Cin = cv.C; a.stride = cv.stride; a.OH = cv.OH; a.OW = cv.OW;
  a.slices = slices; a.per_slice = per_slice; a.items = items;
  a.xcd_group = (per_slice * slices) % (8 * slices) == 0 && per_slice % 8 == 0;
  a.a_bytes = (unsigned)a_bytes;
  a.st = sat_launch_stamps();
  const dim3 grid(per_slice * slices);
  const bool res = g.add1 != nullptr;
  if (NB == 2) {
    switch (K) {
      case 64: launch_kt<2, 4, 2>(res, strided, g.act, grid, s, a); break;
      case 128: launch_kt<4, 2, 2>(res, strided, g.act, grid, s, a); break;
      case 256: launch_kt<8, SAT_STREAM_MB256, 2>(res, strided, g.act, grid, s, a); break;
      default: launch_kt<16, 2, 2>(res, strided, g.act, grid, s, a); break;
    }
  } else {
    switch (K) {
      case 64: launch_kt<2, 4, 1>(res, strided, g.act, grid, s, a); break;
      case 128: launch_kt<4, 4, 1>(res, strided, g.act, grid, s, a); break;
      case 256: launch_kt<8, 4, 1>(res, strided, g.act, grid, s, a); break;
      default: launch_kt<16, 2, 1>(res, strided, g.act, grid, s, a); break;
    }
  }
  *err = (int)hipGetLastError();
  return 1;
}

// ---- chained form: a bottleneck's c3 + residual + ReLU and the next bottleneck's c1 + ReLU in one launch ----
namespace {

// the instantiations: (K, N -> N2) = (64, 256 -> 64), (64, 256 -> 128) [ResNet152 layer1, and into layer2],
// (128, 512 -> 128) [layer2]; 0 = none.  Auto mode takes HBM-bound problems only (sat_conv_stream_try's rule)
int chain_items(long M, int K, int N, int N2, int dtype) {
  if (dtype != SAT_BF16 || M <= 0) return 0;
  const bool l1 = K == 64 && N == 256 && (N2 == 64 || N2 == 128), l2 = K == 128 && N == 512 && N2 == 128;
  if (!l1 && !l2) return 0;
  if (M * N >= (1L << 31)) return 0;   // 32-bit element / buffer offsets
  const int mode = sat_policy().conv_stream;
  if (mode == 1) return 0;
  const int cus = stream_cus();
  if (cus == 0) return 0;
  const int items = sat_cdiv(M, l1 ? 64 : 32);
  if (mode == 0 && items < 2L * cus) return 0;
  return items;
}

}  // namespace

extern "C" int sat_conv1x1_chain_supported(int64_t M, int K, int N, int N2, int dtype, const SatPolicy* policy) {
  SatPolicyScope scope(policy);
  return chain_items(M, K, N, N2, dtype) > 0;
}

extern "C" int sat_conv1x1_chain(int64_t M, int K, int N, int N2, int dtype, const void* x, const void* w,
                                 const float* bias, const void* residual, void* y, const void* w1, const float* b1,
                                 void* x1, const SatPolicy* policy, void* stream) {
  SAT_REQUIRE(M > 0 && M < (1L << 31) && K > 0 && N > 0 && N2 > 0 && x && w && y && w1 && x1);
  SatPolicyScope scope(policy);
  hipStream_t s = (hipStream_t)stream;
  const int items = chain_items(M, K, N, N2, dtype);
  const bool ok = items > 0 && residual && sat_al16(x) && sat_al16(w) && sat_al16(y) && sat_al16(residual) &&
                  sat_al16(w1) && sat_al16(x1) && sat_al16(bias) && sat_al16(b1);   // bias, b1: null passes
  if (!ok) {   // the two launches the chained kernel stands for, through the library's own dispatch
    SatGemm g;
    g.conv = SatConvGeom{1, 1, (int)M, K, 1, 1, 1, 0, 1, (int)M};
    g.M = (int)M; g.N = N; g.K = K; g.dtype = dtype;
    g.A = x; g.B = w; g.ldb = K; g.C = y; g.ldc = N; g.c_dtype = dtype;
    g.bias = bias; g.add1 = residual; g.ld_add1 = N; g.add1_dtype = dtype; g.act = SAT_ACT_RELU;
    const int e = sat_gemm_launch(g, s);
    if (e) return e;
    SatGemm h;
    h.conv = SatConvGeom{1, 1, (int)M, N, 1, 1, 1, 0, 1, (int)M};
    h.M = (int)M; h.N = N2; h.K = N; h.dtype = dtype;
    h.A = y; h.B = w1; h.ldb = N; h.C = x1; h.ldc = N2; h.c_dtype = dtype;
    h.bias = b1; h.act = SAT_ACT_RELU;
    return sat_gemm_launch(h, s);
  }
  const int cus = stream_cus();
  SArgs a{};
  a.M = (int)M; a.N = N; a.K = K;
  a.A = (const bf16*)x; a.B = (const bf16*)w; a.C = (bf16*)y;
  a.bias = bias; a.res = (const bf16*)residual;
  a.H = 1; a.W = (int)M; a.Cin = K; a.stride = 1; a.OH = 1; a.OW = (int)M;
  a.slices = 1; a.per_slice = cus < items ? cus : items; a.items = items;
  a.xcd_group = 0;
  a.a_bytes = (unsigned)(2L * M * K);
  // each output keeps the store policy of its separate launch: y sat_conv_stream_try's rule; x1 the same rule when
  // the stream kernel runs that c1 (N2 = 128), the tile kernel's write-through stores at N2 = 64
  a.wt = 2L * M * N <= (long)SAT_STREAM_WT_BYTES;
  a.B2 = (const bf16*)w1; a.bias2 = b1; a.C2 = (bf16*)x1;
  a.wt2 = N2 < S_BN || 2L * M * N2 <= (long)SAT_STREAM_WT_BYTES;
  a.st = sat_launch_stamps();
  const dim3 grid(a.per_slice), block(S_NW * 64);
  if (K == 64 && N2 == 64) hipLaunchKernelGGL((conv1x1_chain_kernel<2, 4, 2, 4>), grid, block, 0, s, a);
  else if (K == 64) hipLaunchKernelGGL((conv1x1_chain_kernel<2, 4, 2, 8>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv1x1_chain_kernel<4, 2, 4, 8>), grid, block, 0, s, a);
  return (int)hipGetLastError();
}

// ---- projection forms: the stage's first bottleneck, its downsample conv computed inside the c3 launch ----
namespace {

// the instantiations: (K, N, KP, stride, N2) = (64, 256, 64, 1, 0 | 64) [ResNet152 layer1 block 0, plain and chained
// into block 1's c1], (128, 512, 256, 2, 0) [layer2 block 0]; 0 = none, else the item count.  The chained
// (128, 512 -> 128) kernel holds 254 VGPRs without the 64 of the downsample weights: it keeps its separate launch.
int proj_items(long M, int K, int N, int KP, int stride, int N2, int dtype) {
  if (dtype != SAT_BF16 || M <= 0) return 0;
  const bool l1 = K == 64 && N == 256 && KP == 64 && stride == 1 && (N2 == 0 || N2 == 64);
  const bool l2 = K == 128 && N == 512 && KP == 256 && stride == 2 && N2 == 0;
  if (!l1 && !l2) return 0;
  if (M * N >= (1L << 31)) return 0;   // 32-bit element / buffer offsets
  if (N2 > 0) return chain_items(M, K, N, N2, dtype);
  const int mode = sat_policy().conv_stream;
  if (mode == 1) return 0;
  const int cus = stream_cus();
  if (cus == 0) return 0;
  const int items = sat_cdiv(M, l1 ? 64 : 32), slices = N / (2 * S_BN);
  if (mode == 0 && (long)items * slices < 2L * cus) return 0;   // sat_conv_stream_try's rule
  return items;
}

}  // namespace

extern "C" int sat_conv1x1_proj_supported(int64_t M, int K, int N, int Kp, int stride, int N2, int dtype,
                                          const SatPolicy* policy) {
  SatPolicyScope scope(policy);
  return proj_items(M, K, N, Kp, stride, N2, dtype) > 0;
}

extern "C" int sat_conv1x1_proj(int n, int H, int W, int stride, int K, int N, int Kp, int N2, int dtype,
                                const void* x, const void* w, const float* bias, const void* xin, const void* wp,
                                const float* bp, void* y, const void* w1, const float* b1, void* x1,
                                const SatPolicy* policy, void* stream) {
  SAT_REQUIRE(n > 0 && H > 0 && W > 0 && stride > 0 && K > 0 && N > 0 && Kp > 0 && N2 >= 0 && x && w && xin && wp && y);
  SAT_REQUIRE(N2 == 0 || (w1 && x1));
  SatPolicyScope scope(policy);
  hipStream_t s = (hipStream_t)stream;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long M = (long)n * OH * OW, p_bytes = 2L * n * H * W * Kp;
  const int items = M < (1L << 31) ? proj_items(M, K, N, Kp, stride, N2, dtype) : 0;
  // no second path here: the caller issues the downsample launch itself where this one does not apply
  SAT_REQUIRE(items > 0 && p_bytes < (1L << 31));
  SAT_REQUIRE(sat_al16(x) && sat_al16(w) && sat_al16(xin) && sat_al16(wp) && sat_al16(y) && sat_al16(bias) &&
              sat_al16(bp) && sat_al16(w1) && sat_al16(x1) && sat_al16(b1));   // null passes
  const int cus = stream_cus();
  SArgs a{};
  a.M = (int)M; a.N = N; a.K = K;
  a.A = (const bf16*)x; a.B = (const bf16*)w; a.C = (bf16*)y;
  a.bias = bias;
  a.H = 1; a.W = (int)M; a.Cin = K; a.stride = 1; a.OH = 1; a.OW = (int)M;
  a.a_bytes = (unsigned)(2L * M * K);
  a.P = (const bf16*)xin; a.BP = (const bf16*)wp; a.biasP = bp;
  a.pH = H; a.pW = W; a.pstride = stride; a.pOH = OH; a.pOW = OW;
  a.p_bytes = (unsigned)p_bytes;
  a.wt = 2L * M * N <= (long)SAT_STREAM_WT_BYTES;
  a.items = items;
  const dim3 block(S_NW * 64);
  if (N2 > 0) {   // sat_conv1x1_chain's launch
    a.slices = 1; a.per_slice = cus < items ? cus : items;
    a.xcd_group = 0;
    a.B2 = (const bf16*)w1; a.bias2 = b1; a.C2 = (bf16*)x1;
    a.wt2 = N2 < S_BN || 2L * M * N2 <= (long)SAT_STREAM_WT_BYTES;
    a.st = sat_launch_stamps();
    hipLaunchKernelGGL((conv1x1_proj_kernel<2, 4, 2, 4, 2, false>), dim3(a.per_slice), block, 0, s, a);
    return (int)hipGetLastError();
  }
  // sat_conv_stream_try's launch of the same c3 (256-column slices, one workgroup per CU)
  const int slices = N / (2 * S_BN);
  int per_slice = cus / slices;
  if (per_slice < 1) per_slice = 1;
  if (per_slice > items) per_slice = items;
  a.slices = slices; a.per_slice = per_slice;
  a.xcd_group = (per_slice * slices) % (8 * slices) == 0 && per_slice % 8 == 0;
  a.st = sat_launch_stamps();
  const dim3 grid(per_slice * slices);
  if (K == 64) hipLaunchKernelGGL((conv1x1_proj_kernel<2, 4, 2, 0, 2, false>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv1x1_proj_kernel<4, 2, 2, 0, 8, true>), grid, block, 0, s, a);
  return (int)hipGetLastError();
}

// Weight gradient of a 3x3 / stride-1 / pad-1 convolution on NHWC bf16 tensors, for gfx950 (MI355X): what autograd
// computes for conv.weight when the top of the encoder trunk is trained -- the c2 of a torchvision Bottleneck
// (Bottleneck.forward, reached through encoder.py:13-17) and VGG19's block-5 convolutions (encoder.py:24-27).
//
//   dW[co][kh][kw][ci] = sum over (n, oh, ow) of dZ[n, oh, ow, co] * X[n, oh + kh - 1, ow + kw - 1, ci]
//
// bf16 operands, fp32 accumulation, fp32 output in the folded weight's own [Cout][3][3][Cin] order (+ dW when
// accumulating).  As a GEMM: M = Cout, N = 9 Cin, K = n H W pixels, and both operands are k-major (a pixel's
// channels are contiguous), the form split_gemm_kernel (gemmsplit.hip) stages with ds_read_b64_tr_b16.  This kernel
// is that one with an implicit-im2col B loader:
//   * Cin % 128 == 0, so a 128-column n-tile lies inside ONE tap (kh, kw): the tap is uniform per workgroup, and
//     k-row p of B is pixel p of X shifted by (kh - 1) W + (kw - 1) -- the same 256-B rows, a different start.  Rows
//     whose shifted position leaves the image (the padding), and rows past K, take the offset kSatOOB and land as
//     zeros: no branch, no zero line.  A lane decodes its rows' p -> (oh, ow) per k-tile (two rows per lane at 128
//     columns: the two 1-KiB DMA instructions a wave issues for B);
//   * everything else as gemmsplit.hip: BM x 128 x 64 tiles (BM = 128 or 256), a 3-stage LDS ring filled by
//     buffer_load ... lds, one counted vmcnt + raw s_barrier per k-tile with tile t+2 in flight, sat_frag_kmajor
//     fragment reads, XCD-aware tile order, and deterministic split-K -- write-through partial tiles, one arrival
//     ticket per output tile, the last arriver sums the partials in split order (no fp32 atomics; bit-identical run
//     to run).  The hand-off is gemmsplit.hip's fence-free form, under the same conditions: 16-B sc1 stores drained
//     by every storing wave before the barrier, one lane's agent-scope ticket add, 16-B sc1 loads after the barrier
//     that lane joins, a hipMalloc'd workspace, and one workgroup resident per CU (96 / 144 KiB of LDS each).
// Unlike the decoder's products this one may run more workgroups than CUs (144 output tiles at 512 channels): the
// last arriver never waits for anybody, so later rounds need no co-residency.
// fp32 operands (parity mode) take no kernel of their own: a gather of the im2col matrix and the exact fp32 GEMM.
#include "sat_common.h"
#include "sat_internal.h"
#include "sat_lds_pipe.h"

namespace {

constexpr int WBN = 128, WBK = 64, WNSTG = 3;
constexpr int kMaxSplits = 8;
constexpr int kCUs = 256;
constexpr long kMaxSlabBytes = 32L << 20;   // partial tiles of one launch (512 of 128 x 128)

template <int BM>
struct WGeom {
  static constexpr int WGN = BM == 256 ? 2 : 4;   // waves along N
  static constexpr int WGM = 8 / WGN;
  static constexpr int WTM = BM / WGM, WTN = WBN / WGN;
  static constexpr int MI = WTM / 16, NJ = WTN / 16;
  static constexpr int STAGE_A = BM * WBK * 2, STAGE_B = WBN * WBK * 2, STAGE = STAGE_A + STAGE_B;
  static constexpr int AI = STAGE_A / 1024 / 8, BI = STAGE_B / 1024 / 8, INSTR = AI + BI;   // 1 KiB DMAs per wave
  static constexpr int EPI_LD = WBN + 4;
  static constexpr int EPI_BYTES = BM * EPI_LD * 4;
  static constexpr int LDS = WNSTG * STAGE;
  static_assert(WTM == 64 && MI == 4, "wave tiles are 64 rows high");
  static_assert(BI == 2, "two B rows per lane and k-tile");
  static_assert(EPI_BYTES + 16 <= LDS, "epilogue tile + ticket word must fit in the ring");
};

struct WArgs {
  int H, W, HW, Cin, Cout, K;   // K = n H W pixels
  const bf16* dz;               // [K][Cout]
  const bf16* x;                // [K][Cin]
  float* dw;                    // [Cout][9 Cin]
  int beta1;                    // dw += product
  int splits, kchunk;           // split s: pixels [s kchunk, min(K, (s + 1) kchunk)), kchunk a multiple of WBK
  int tiles_m, tiles_n;
  unsigned dz_bytes, x_bytes, dw_bytes, slab_bytes;
  float* slab;                  // splits > 1: [tile][split][BM x WBN] partials in the accumulator layout
  unsigned* tickets;            // splits > 1: one arrival counter per tile, zero at launch
  SatStamps st;
};

__device__ __forceinline__ uint4 f4u(f32x4 v) {
  return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}

template <int BM>
__device__ __forceinline__ void wgrad_body(const WArgs& a) {
  using G = WGeom<BM>;
  constexpr int MI = G::MI, NJ = G::NJ, AI = G::AI, BI = G::BI;
  __shared__ __attribute__((aligned(16))) char smem[G::LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / G::WGN, wn = w % G::WGN;

  // XCD-aware order: each XCD takes a contiguous run of (split, m-tile, n-tile) indices, so the workgroups on one
  // XCD share their dZ panel and neighbouring taps of X
  const int lin = sat_xcd_tile(blockIdx.x, gridDim.x);
  const int nt = lin % a.tiles_n;
  const int rest = lin / a.tiles_n;
  const int mt = rest % a.tiles_m, split = rest / a.tiles_m;
  const int m0 = mt * BM, n0 = nt * WBN;
  const int M = a.Cout, N = 9 * a.Cin;
  const int kbeg = split * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  const int nk = kend > kbeg ? (kend - kbeg + WBK - 1) / WBK : 0;
  // the workgroup's tap and first input channel: n = (kh 3 + kw) Cin + ci
  const int tap = n0 / a.Cin, ci0 = n0 - tap * a.Cin;
  const int dh = tap / 3 - 1, dwid = tap % 3 - 1;
  const int shift = dh * a.W + dwid;

  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)a.dz, (short)0, (int)a.dz_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)a.x_bytes, 0x00020000);
  // per-lane DMA pieces, fixed across k-tiles (4 k-rows of 256 B per 1 KiB instruction: lane -> k-row lane >> 4,
  // slot lane & 15): the column and the k-row within the tile
  int a_off[AI], a_k[AI];
  bool a_ok[AI];
#pragma unroll
  for (int j = 0; j < AI; ++j) {
    const int q = (w * AI + j) * 4 + (lane >> 4);   // half q >> 6 (128 m each), k-row q & 63
    const int kr = q & 63, ch = (lane & 15) ^ sat_swz256(kr);
    const int m = m0 + (q >> 6) * 128 + 8 * ch;
    a_ok[j] = m + 8 <= M;
    a_off[j] = m;
    a_k[j] = kr;
  }
  int b_off[BI], b_k[BI];
#pragma unroll
  for (int j = 0; j < BI; ++j) {
    const int kr = (w * BI + j) * 4 + (lane >> 4), ch = (lane & 15) ^ sat_swz256(kr);
    b_off[j] = ci0 + 8 * ch;   // < Cin: the tile lies inside one tap
    b_k[j] = kr;
  }
  auto stage = [&](int buf, int k0) {
    char* sa = smem + buf * G::STAGE;
    char* sb = sa + G::STAGE_A;
#pragma unroll
    for (int j = 0; j < AI; ++j) {
      const int k = k0 + a_k[j];
      const bool ok = a_ok[j] && k < kend;
      const unsigned off = 2u * (unsigned)((long)k * a.Cout + a_off[j]);
      sat_bdma16(rA, sa + (w * AI + j) * 1024, ok ? off : kSatOOB);
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
      const int p = k0 + b_k[j];   // output pixel (n, oh, ow) of this k-row
      const unsigned rem = (unsigned)p % (unsigned)a.HW;
      const int oh = (int)(rem / (unsigned)a.W), ow = (int)(rem - (unsigned)oh * (unsigned)a.W);
      const int ih = oh + dh, iw = ow + dwid;
      const bool ok = p < kend && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
      const unsigned off = 2u * (unsigned)((long)(p + shift) * a.Cin + b_off[j]);
      sat_bdma16(rB, sb + (w * BI + j) * 1024, ok ? off : kSatOOB);
    }
  };

  // fragments of 32-deep half h of the tile in buf
  const int fr = lane & 15, fh = lane >> 4;
  const int am = wm * G::WTM;   // the wave's first row in the tile
  auto frags = [&](int buf, int h, bf16x8 (&fa)[MI], bf16x8 (&fb)[NJ]) {
    const char* sa = smem + buf * G::STAGE;
    const char* sb = sa + G::STAGE_A;
#pragma unroll
    for (int i = 0; i < MI; ++i) fa[i] = sat_frag_kmajor(sa + (am >> 7) * (64 * 256), h * 32, (am & 127) + i * 16, lane);
#pragma unroll
    for (int j = 0; j < NJ; ++j) fb[j] = sat_frag_kmajor(sb, h * 32, wn * G::WTN + j * 16, lane);
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
      stage(1, kbeg + WBK);
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
      if (dma) stage(cur == 0 ? 2 : cur - 1, kbeg + (t + 2) * WBK);
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
    constexpr unsigned PART = (unsigned)BM * WBN * 4;   // bytes of one partial tile
    const unsigned tbase = (unsigned)(tile * a.splits) * PART;
    auto slot = [&](int i, int j) { return (unsigned)((((w * MI + i) * NJ + j) * 64 + lane) * 16); };
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) sat_st16<16>(rS, tbase + (unsigned)split * PART + slot(i, j), f4u(acc[i][j]));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave: its write-through stores are done
    __syncthreads();
    volatile unsigned* flag = (volatile unsigned*)(smem + G::EPI_BYTES);
    if (tid == 0)
      *flag = __hip_atomic_fetch_add(a.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

  // ---- dW: the fp32 tile through LDS, 16-B row pieces (beta = 1 adds dW) ----
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
  if (col >= N) return;
  const __amdgpu_buffer_rsrc_t rC = sat_out_rsrc(a.dw, a.dw_bytes);
#pragma unroll
  for (int it = 0; it < BM / 32; ++it) {
    const int rl = r0 + it * 32, row = m0 + rl;
    if (row >= M) break;
    float4 x0 = *(const float4*)(ep + rl * G::EPI_LD + cc * 8);
    float4 x1 = *(const float4*)(ep + rl * G::EPI_LD + cc * 8 + 4);
    const unsigned off = (unsigned)(((long)row * N + col) * 4);
    if (a.beta1) {
      const float* p = a.dw + (long)row * N + col;
      x0 = f4add(x0, *(const float4*)p);
      x1 = f4add(x1, *(const float4*)(p + 4));
    }
    sat_st16<0>(rC, off, make_uint4(__float_as_uint(x0.x), __float_as_uint(x0.y), __float_as_uint(x0.z), __float_as_uint(x0.w)));
    sat_st16<0>(rC, off + 16, make_uint4(__float_as_uint(x1.x), __float_as_uint(x1.y), __float_as_uint(x1.z), __float_as_uint(x1.w)));
  }
}

template <int BM>
__global__ __launch_bounds__(512) void conv3x3_wgrad_kernel(WArgs a) {
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  wgrad_body<BM>(a);
  sat_stamp_end(a.st, t0);
}

struct WPlan {
  int bm = 0, splits = 1, kchunk = 0, tiles_m = 0, tiles_n = 0;
  long slab_bytes = 0;
};

// The split GEMM's cost model (gemmsplit.hip plan_split: microseconds per k-tile of a workgroup, the C epilogue,
// a partial tile read by the last arriver), over rounds of one workgroup per CU.  `force` = SatPolicy::split_k: that
// split count where the shape allows it (at least one k-tile per split, no empty split), else the model's choice.
constexpr double kKtileUs[2] = {0.73, 1.10};   // BM = 128, 256
constexpr double kEpiUs = 1.0;
constexpr double kPartUs[2] = {0.94, 1.87};
WPlan plan_wgrad(int Cin, int Cout, long K, bool have_ws, int force) {
  const int nk = sat_cdiv(K, WBK);
  WPlan best;
  double best_us = 1e30;
  for (int b = 0; b < 2; ++b) {
    const int bm = b ? 256 : 128;
    const int tm = sat_cdiv(Cout, bm), tn = 9 * Cin / WBN;
    const long tiles = (long)tm * tn;
    for (int s = 1; s <= kMaxSplits; ++s) {
      if (force > 0 && s != force) continue;
      const long slab = tiles * s * bm * WBN * 4;
      if (s > 1 && (!have_ws || tiles > (long)kSatSplitTickets || slab > kMaxSlabBytes || nk < (force > 0 ? s : 2 * s)))
        continue;
      const int kch = sat_cdiv(nk, s);
      if (sat_cdiv(nk, kch) != s) continue;   // no empty split
      const double us = sat_cdiv(tiles * s, kCUs) * (kch * kKtileUs[b] + kEpiUs) + (s - 1) * kPartUs[b];
      if (us < best_us - 1e-9) {
        best.bm = bm; best.splits = s; best.kchunk = kch * WBK; best.tiles_m = tm; best.tiles_n = tn;
        best.slab_bytes = s > 1 ? slab : 0;
        best_us = us;
      }
    }
  }
  if (best.bm == 0 && force > 0) return plan_wgrad(Cin, Cout, K, have_ws, 0);
  return best;
}

// fp32 (the parity path, not a performance path): gather the im2col matrix [K][9 Cin] and run the exact fp32 GEMM on it
__global__ void im2col3x3_f32_kernel(const float* __restrict__ x, float* __restrict__ cols, int H, int W, int Cin, long K) {
  const int c4 = Cin / 4;
  const long total = K * 9 * c4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % c4);
    const long r = i / c4;
    const int tap = (int)(r % 9);
    const long p = r / 9;
    const int rem = (int)(p % ((long)H * W)), oh = rem / W, ow = rem - oh * W;
    const int ih = oh + tap / 3 - 1, iw = ow + tap % 3 - 1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
      v = ((const float4*)(x + (p + (long)(tap / 3 - 1) * W + (tap % 3 - 1)) * Cin))[c];
    ((float4*)(cols + (p * 9 + tap) * Cin))[c] = v;
  }
}

bool wgrad_shape_ok(int N, int H, int W, int Cin, int Cout, int dtype) {
  if (dtype == SAT_F32)   // the im2col matrix under 2 GiB
    return N >= 1 && H >= 1 && W >= 1 && Cin >= 128 && Cout >= 128 && Cin % 128 == 0 && Cout % 128 == 0 &&
           36L * N * H * W * Cin < (1L << 31) && 4L * N * H * W * Cout < (1L << 31) && 36L * Cin * Cout < (1L << 31);
  if (dtype != SAT_BF16 || N < 1 || H < 1 || W < 1 || Cin < 128 || Cout < 128 || Cin % 128 || Cout % 128) return false;
  // buffer offsets are 32-bit: both operands and dW below 2 GiB
  const long K = (long)N * H * W;
  return 2L * K * Cin < (1L << 31) && 2L * K * Cout < (1L << 31) && 36L * Cin * Cout < (1L << 31);
}

}  // namespace

/* see include/sat_hip.h */
extern "C" size_t sat_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype,
                                                    const SatPolicy* policy) {
  if (!wgrad_shape_ok(N, H, W, Cin, Cout, dtype)) return 0;
  if (dtype == SAT_F32) return (size_t)36 * N * H * W * Cin;
  const WPlan p = plan_wgrad(Cin, Cout, (long)N * H * W, true, policy ? policy->split_k : 0);
  return (size_t)p.slab_bytes + kSatSplitTickets * 4;
}

extern "C" int sat_conv3x3_wgrad(int N, int H, int W, int Cin, int Cout, int dtype, const void* x, const void* dz,
                                 float* dw, int accumulate, void* workspace, size_t workspace_bytes,
                                 const SatPolicy* policy, void* stream) {
  SAT_REQUIRE(x && dz && dw && wgrad_shape_ok(N, H, W, Cin, Cout, dtype));
  SAT_REQUIRE(sat_al16(x) && sat_al16(dz) && sat_al16(dw) && sat_al16(workspace));
  SatPolicyScope scope(policy);
  hipStream_t s = (hipStream_t)stream;
  const long K = (long)N * H * W;
  if (dtype == SAT_F32) {
    SAT_REQUIRE(workspace && workspace_bytes >= (size_t)36 * K * Cin);
    float* cols = (float*)workspace;
    const long total = K * 9 * (Cin / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(im2col3x3_f32_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s,
                       (const float*)x, cols, H, W, Cin, K);
    SAT_LAUNCH_CHECK();
    SatGemm g;   // dw [Cout][9 Cin] = dz^T cols: both operands k-major
    g.M = Cout; g.N = 9 * Cin; g.K = (int)K; g.dtype = SAT_F32;
    g.A = dz; g.lda = Cout; g.transA = 1;
    g.B = cols; g.ldb = 9 * Cin; g.transB = 1;
    g.C = dw; g.ldc = 9 * Cin; g.c_dtype = SAT_F32;
    g.beta = accumulate ? 1.f : 0.f;
    return sat_gemm_launch(g, s);
  }
  const WPlan p = plan_wgrad(Cin, Cout, K, workspace != nullptr, policy ? policy->split_k : 0);
  SAT_REQUIRE(p.bm != 0);
  WArgs a{};
  a.H = H; a.W = W; a.HW = H * W; a.Cin = Cin; a.Cout = Cout; a.K = (int)K;
  a.dz = (const bf16*)dz; a.x = (const bf16*)x; a.dw = dw;
  a.beta1 = accumulate != 0;
  a.splits = p.splits; a.kchunk = p.kchunk; a.tiles_m = p.tiles_m; a.tiles_n = p.tiles_n;
  a.dz_bytes = (unsigned)(2L * K * Cout); a.x_bytes = (unsigned)(2L * K * Cin);
  a.dw_bytes = (unsigned)(36L * Cin * Cout);
  const long tiles = (long)p.tiles_m * p.tiles_n;
  if (p.splits > 1) {
    // [partial tiles | tickets]; the tickets are zeroed here, on the stream (a kernel: capturable)
    SAT_REQUIRE(workspace_bytes >= (size_t)p.slab_bytes + kSatSplitTickets * 4 && tiles <= (long)kSatSplitTickets);
    a.slab = (float*)workspace; a.slab_bytes = (unsigned)p.slab_bytes;
    a.tickets = (unsigned*)((char*)workspace + p.slab_bytes);
    SAT_CHECK((hipError_t)sat_zero_rows((float*)a.tickets, tiles, 1, tiles, s));
  }
  a.st = sat_launch_stamps();
  const dim3 grid((unsigned)(tiles * p.splits));
  if (p.bm == 256) hipLaunchKernelGGL((conv3x3_wgrad_kernel<256>), grid, dim3(512), 0, s, a);
  else hipLaunchKernelGGL((conv3x3_wgrad_kernel<128>), grid, dim3(512), 0, s, a);
  SAT_LAUNCH_CHECK();
  return 0;
}

// Weight-stationary 3x3 convolution for 64 -> 64 channels (gfx950 / MI355X).
//
//   y = act(conv3x3(x, w, stride 1, pad 1) + bias),  x / y NHWC bf16 with C = Cout = 64, fp32 accumulation
//
// Shapes: ResNet152 layer1's c2 (56 x 56, 3 launches per forward) and VGG19's conv1_2 (224 x 224, the
// largest launch of that trunk: 473 GFLOP per 128 images) -- encoder.py:13-17,23-27 through
// torchvision.  On the 128 x 64 implicit-GEMM tile kernel these ran at ~0.2 of the MFMA peak: each
// tile re-fetched its 128 output pixels' input rows once per filter tap (9 x 16 KB of A plus 8 KB of
// weights per 64-deep k-tile) through the CU's ~50 GB/s LDS-DMA intake.  Here:
//   * one persistent 8-wave workgroup per CU (two waves per SIMD: one wave's fragment reads hide
//     behind the other's MFMAs -- with one wave per SIMD the loop ran at a fifth of the MFMA rate,
//     waiting on every ds_read); wave w owns output channels 16 (w % 4) .. +15 of half the item's
//     pixels and keeps the weight fragments of its channels for all K = 9 x 64 in VGPRs for the whole
//     kernel (18 x 16 B per lane), so the only bytes streamed per item are activations;
//   * an item is 224 output pixels (4 image rows of 56, or 2 x 112 of a 224-wide image); its input
//     halo ((rows + 2) x (cols + 2) pixels of 128 B, zero outside the image through out-of-range
//     buffer offsets) lands in LDS ONCE by LDS-DMA and every tap reads it shifted: 45-58 KB per item
//     instead of 9 x 56 KB;
//   * ring of NSTG stages (3 at width 56, 2 at width 224), counted vmcnt across one barrier per item
//     (the previous items' stores stay in flight), as in convstream.hip;
//   * LDS image swizzled on the source: 16-B chunk c of pixel row r at slot c ^ (r & 7), so the 16
//     pixels an MFMA fragment reads under any tap shift hit distinct bank groups;
//   * C^T = W . X^T on v_mfma_f32_16x16x32_bf16: a lane ends with 4 consecutive channels of one pixel;
//     bias, activation and one bf16 rounding, 8-B stores.
// Summation order: k ascending (tap-major, channel within tap) like the tile kernel's k-loop, so the
// fp32 sums differ from it only by the MFMA's internal 32-deep grouping (same instruction, same k
// grouping): results are bit-identical to the tile kernel (tests/test_gpu_parity.py).
#include "sat_common.h"
#include "sat_internal.h"
#include "sat_lds_pipe.h"

namespace {

constexpr int WS_NW = 8;                 // waves per workgroup: 4 channel groups x 2 pixel halves
constexpr int WS_NOUT = 64;              // output channels (4 groups of 16)
constexpr int WS_MB = 7;                 // 16-pixel m-blocks per wave (112 of the item's 224 pixels)

struct WArgs {
  const bf16* x; const bf16* w; const float* bias; bf16* y;
  int N, H, W;                           // images, height, width (= output height, width)
  int items, items_per_img, tiles_x;     // items = N * (H / TR) * tiles_x
  unsigned x_bytes, y_bytes;
  SatStamps st;                      // in-kernel launch timestamps (SatPolicy::stamps)
};

// KK x KK window with PADT rows / columns of top-left padding over C input channels (3 / 64 / 1: the
// 3x3 convs; 4 / 16 / 2: ResNet152's stem as a 4x4 conv over the 2x2 space-to-depth input);
// TR x TW output pixels per item (TR * TW = 224); HP halo pixels, DMA rounds of 8 KB (16 B per lane)
template <int KK, int C, int PADT, int TR, int TW, int NSTG, int ACT>
__device__ __forceinline__ void conv_ws_kernel_body(const WArgs& a) {
  static_assert(TR * TW == 2 * WS_MB * 16, "224 pixels per item");
  static_assert(NSTG == 2 || NSTG == 3, "ring depth");
  static_assert(C == 64 || C == 16, "8 or 2 16-B chunks per pixel");
  constexpr int K = KK * KK * C, KSN = K / 32;             // k-steps of 32
  constexpr int CPX = C / 8;                               // 16-B chunks per halo pixel
  constexpr int HW_ = TW + KK - 1, HP = (TR + KK - 1) * HW_;
  constexpr int ROWB = C * 2;                              // bytes per halo pixel
  constexpr int NDMA = (HP * ROWB + WS_NW * 1024 - 1) / (WS_NW * 1024);   // DMA instructions per lane per item
  constexpr int STG = NDMA * WS_NW * 1024;                 // LDS bytes per stage
  static_assert(NSTG * STG <= 160 * 1024, "ring fits in LDS");
  constexpr int ST = WS_MB;                                // 8-B stores per lane per item
  __shared__ __attribute__((aligned(16))) char smem[NSTG * STG];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = w & 3, ph = w >> 2;                      // channel group, pixel half
  const int fr = lane & 15, fh = lane >> 4;

  // weight fragments of this wave's 16 channels for all of K (k = tap * C + ci), loaded once
  bf16x8 bq[KSN];
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) bq[ks] = *(const bf16x8*)(a.w + (long)(16 * cg + fr) * K + ks * 32 + 8 * fh);
  float bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias4[j] = a.bias ? a.bias[16 * cg + 4 * fh + j] : 0.f;
  // consume the weights and biases here: otherwise the compiler's vmcnt tracking still sees them
  // pending inside the item loop and inserts waits that also drain the next items' halo DMAs
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) asm volatile("" ::"v"(bq[ks]));
#pragma unroll
  for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(bias4[j]));

  const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rY = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, (short)0, (int)a.y_bytes, 0x00020000);

  auto item_origin = [&](int it, int& n, int& y0, int& x0) {
    n = it / a.items_per_img;
    const int r = it - n * a.items_per_img;
    const int ty = r / a.tiles_x;
    y0 = ty * TR;
    x0 = (r - ty * a.tiles_x) * TW;
  };
  // halo of item `it` into stage `buf`: LDS byte b = (d * NW + w) * 1024 + lane * 16 holds chunk
  // pc = (b % ROWB) / 16 of halo pixel hp = b / ROWB, i.e. logical chunk c = pc ^ (hp & 7) (C = 64;
  // two chunks per pixel at C = 16 need no swizzle)
  auto stage = [&](int it, int buf) {
    int n, y0, x0;
    item_origin(it, n, y0, x0);
    char* st = smem + buf * STG;
#pragma unroll
    for (int d = 0; d < NDMA; ++d) {
      const int byte = (d * WS_NW + w) * 1024 + lane * 16;
      const int hp = byte / ROWB, pc = (byte % ROWB) >> 4, c = CPX == 8 ? pc ^ (hp & 7) : pc;
      const int hy = hp / HW_, hx = hp - hy * HW_;
      const int yy = y0 + hy - PADT, xx = x0 + hx - PADT;
      const bool ok = hp < HP && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      const unsigned off = ok ? (unsigned)(((((long)n * a.H + yy) * a.W + xx) * C + 8 * c) * 2) : kSatOOB;
      sat_bdma16(rX, st + (d * WS_NW + w) * 1024, off);
    }
  };
  // the halo pixel of output pixel i*16 + fr under tap (kh, kw) = hp0[i] + kh * HW_ + kw
  int hp0[WS_MB];
#pragma unroll
  for (int i = 0; i < WS_MB; ++i) {
    const int p = (ph * WS_MB + i) * 16 + fr, py = p / TW, px = p - py * TW;
    hp0[i] = py * HW_ + px;
  }

  int it = blockIdx.x;
  if (it >= a.items) return;   // workgroup-uniform
  const int step = gridDim.x;
  stage(it, 0);
  if (NSTG == 3 && it + step < a.items) stage(it + step, 1);
  int buf = 0;
  for (int k = 0;; ++k) {
    // this item's DMAs have landed once only younger ops remain: (3 stages) the next item's DMAs and
    // the stores of the previous one or two items, (2 stages) the previous item's stores -- they
    // stay in flight across the barrier
    if constexpr (NSTG == 3) {
      const int younger = (it + step < a.items ? NDMA : 0) + (k >= 1 ? ST : 0) + (k >= 2 ? ST : 0);
      switch (younger) {
        case NDMA + 2 * ST: sat_vm_lds_barrier<NDMA + 2 * ST>(); break;
        case NDMA + ST: sat_vm_lds_barrier<NDMA + ST>(); break;
        case NDMA: sat_vm_lds_barrier<NDMA>(); break;
        case 2 * ST: sat_vm_lds_barrier<2 * ST>(); break;
        case ST: sat_vm_lds_barrier<ST>(); break;
        default: sat_vm_lds_barrier<0>(); break;
      }
      if (it + 2 * step < a.items) stage(it + 2 * step, buf == 0 ? 2 : buf - 1);
    } else {
      if (k >= 1) sat_vm_lds_barrier<ST>();
      else sat_vm_lds_barrier<0>();
      if (it + step < a.items) stage(it + step, buf ^ 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    const char* base = smem + buf * STG;
    // opaque per item: keeps the 126 per-(m-block, tap) LDS addresses from being hoisted out of the
    // item loop into registers (they are a few VALU ops each, recomputed next to their reads)
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) asm volatile("" : "+v"(hp0[i]));
    f32x4 acc[WS_MB];
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto afrag = [&](int i, int ks) {   // k = ks * 32 + 8 fh: tap k / C, chunk (k % C) / 8
      const int k = ks * 32 + 8 * fh, tap = k / C, c = (k % C) >> 3;
      const int hp = hp0[i] + (tap / KK) * HW_ + tap % KK;
      return *(const bf16x8*)(base + hp * ROWB + 16 * (CPX == 8 ? c ^ (hp & 7) : c));
    };
    bf16x8 af[2][WS_MB];
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) af[0][i] = afrag(i, 0);
#pragma unroll
    for (int ks = 0; ks < KSN; ++ks) {
      if (ks + 1 < KSN) {
#pragma unroll
        for (int i = 0; i < WS_MB; ++i) af[(ks + 1) & 1][i] = afrag(i, ks + 1);
      }
#pragma unroll
      for (int i = 0; i < WS_MB; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[ks], af[ks & 1][i], acc[i], 0, 0, 0);
    }
    // epilogue: lane holds channels 16 cg + 4fh .. +3 of output pixel (ph * 7 + i) * 16 + fr
    int n, y0, x0;
    item_origin(it, n, y0, x0);
    auto out_at = [&](int i, unsigned& off) {   // bias + act of m-block i, rounded once; its byte offset
      const int p = (ph * WS_MB + i) * 16 + fr, py = p / TW, px = p - py * TW;
      sat_u32x2 o;
      bf16* ob = (bf16*)&o;
#pragma unroll
      for (int j = 0; j < 4; ++j) ob[j] = (bf16)apply_act(acc[i][j] + bias4[j], ACT);
      off = (unsigned)(((((long)n * a.H + y0 + py) * a.W + x0 + px) * WS_NOUT + 16 * cg + 4 * fh) * 2);
      return o;
    };
    // m-block pairs through 16-B stores (sat_common.h, sat_st_pair16), an odd last one with 8 B; plain write-back
    // here: write-through stores of the stem / layer1 outputs measured slower (6.28-6.31 vs 6.38-6.40 ms per step,
    // profiles/r4_s19)
#pragma unroll
    for (int i = 0; i + 1 < WS_MB; i += 2) {
      unsigned offA, offB;
      const sat_u32x2 oa = out_at(i, offA), ob2 = out_at(i + 1, offB);
      sat_st_pair16<0>(rY, offA, offB, oa, ob2, true, true);
    }
    if constexpr (WS_MB % 2) {
      unsigned off;
      const sat_u32x2 o = out_at(WS_MB - 1, off);
      __builtin_amdgcn_raw_buffer_store_b64(o, rY, (int)off, 0, 0);
    }
    it += step;
    if (it >= a.items) break;
    buf = NSTG == 3 ? (buf == 2 ? 0 : buf + 1) : buf ^ 1;
  }
}

template <int KK, int C, int PADT, int TR, int TW, int NSTG, int ACT>
__global__ __launch_bounds__(WS_NW * 64) void conv_ws_kernel(WArgs a) {
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  conv_ws_kernel_body<KK, C, PADT, TR, TW, NSTG, ACT>(a);
  sat_stamp_end(a.st, t0);
}

// ---- the stem with its 3x3 / stride 2 / pad 1 max pool (ResNet152: conv1 + bn1 + relu + maxpool) in one launch ----
// The stem instantiation <4, 16, 2, 2, 112, 3> already lines up with the pool: an item is conv rows (2q, 2q + 1) of
// one image, wave (cg, ph) owns the whole conv row 2q + ph of its 16 channels, a lane 4 channels of pixel 16 i + fr.
//   * epilogue values first (bias, ReLU, one bf16 rounding -- the conv launch's output, exactly), then the pool
//     on them: what maxpool_bf16_kernel computes from the stored tensor, so the 112 x 112 tensor is never written;
//   * column pool inside the wave: pooled column P = 8 i + fr / 2 (even fr) is the max over pixels fr - 1, fr,
//     fr + 1 -- two lane moves inside the 16-lane row; lane fr = 0 takes pixel 15 of m-block i - 1, which the same
//     move of that m-block delivered to it; column -1 takes no part;
//   * row pool: pooled row q = max of the column-pooled conv rows 2q - 1, 2q, 2q + 1.  Rows 2q - 1 and 2q + 1 belong
//     to the ph = 1 wave (the previous item's and this item's), so a workgroup walks a contiguous run of items of one
//     image and the ph = 1 wave leaves its row in one of two 7 KB exchange buffers behind the ring, alternating by
//     item (the MFMA loop has no registers to carry a row in at four waves per SIMD).  After one LDS-only barrier per
//     item (DMAs and stores stay in flight) the ph = 0 wave reads this item's and the previous item's buffer,
//     combines them with its row 2q and stores pooled row q; row -1 takes no part;
//   * the third DMA round of a halo stage is issued by the two waves whose kilobytes hold halo pixels only, so a
//     stage is 18 KB and ring + exchange stay under 80 KB: two workgroups per CU, as the conv launch has;
//   * a run that does not start at an image top first computes the item above it without storing anything (its second
//     conv row is the first pooled row's row 2q - 1).
// The exchange reads and writes are asm statements: ahead of an LDS access it can see, the compiler waits for the
// LDS-DMAs in flight with a vmcnt(0) of its own (convstream.hip).
struct PArgs {
  const bf16* x; const bf16* w; const float* bias; bf16* y;
  int N, H, W;                           // images, conv height (even), conv width (112)
  int ipi, rl, rpi, runs;                // items (= pooled rows) per image, items per run, runs per image, runs
  unsigned x_bytes, y_bytes;
  SatStamps st;
};

struct PRun {   // a workgroup's position in its runs (workgroup-uniform)
  int run, n, q, q0, qend;
};

__device__ __forceinline__ void conv_stem_pool_kernel_body(const PArgs& a) {
  constexpr int KK = 4, C = 16, PADT = 2, TR = 2, TW = 112, NSTG = 3;
  constexpr int K = KK * KK * C, KSN = K / 32;
  constexpr int HW_ = TW + KK - 1, HP = (TR + KK - 1) * HW_;
  constexpr int ROWB = C * 2;
  constexpr int KB = (HP * ROWB + 1023) / 1024;            // kilobytes (one wave's DMA instruction) of a halo stage
  constexpr int STG = KB * 1024;
  static_assert(KB > 2 * WS_NW && KB < 3 * WS_NW, "two whole DMA rounds and part of a third");
  constexpr int PW = TW / 2;                               // pooled width
  constexpr int XCG = PW * 16 * 2, XB = 4 * XCG;           // exchange bytes per channel group, per buffer
  static_assert(2 * (NSTG * STG + 2 * XB) <= 160 * 1024, "two workgroups per CU");
  constexpr int ST = WS_MB;                                // 8-B stores per lane per item (ph = 0 waves)
  __shared__ __attribute__((aligned(16))) char smem[NSTG * STG + 2 * XB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = w & 3, ph = w >> 2;
  const int fr = lane & 15, fh = lane >> 4;
  const bool dma3 = 2 * WS_NW + w < KB;                    // this wave issues a third DMA per item
  const int ndma = dma3 ? 3 : 2;

  bf16x8 bq[KSN];
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) bq[ks] = *(const bf16x8*)(a.w + (long)(16 * cg + fr) * K + ks * 32 + 8 * fh);
  float bias4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bias4[j] = a.bias ? a.bias[16 * cg + 4 * fh + j] : 0.f;
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) asm volatile("" ::"v"(bq[ks]));
#pragma unroll
  for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(bias4[j]));

  const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, (short)0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rY = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, (short)0, (int)a.y_bytes, 0x00020000);

  const int G = gridDim.x;
  auto open_run = [&](PRun& r) {   // r.run < a.runs
    r.n = r.run / a.rpi;
    r.q0 = (r.run - r.n * a.rpi) * a.rl;
    r.qend = r.q0 + a.rl < a.ipi ? r.q0 + a.rl : a.ipi;
    r.q = r.q0 > 0 ? r.q0 - 1 : 0;   // the item above the run: computed, not stored
  };
  auto advance = [&](PRun& r) {
    if (++r.q == r.qend) {
      r.run += G;
      if (r.run < a.runs) open_run(r);
    }
  };
  auto stage = [&](const PRun& r, int buf) {
    const int y0 = r.q * TR;
    char* st = smem + buf * STG;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d == 2 && !dma3) break;   // wave-uniform
      const int byte = (d * WS_NW + w) * 1024 + lane * 16;
      const int hp = byte / ROWB, pc = (byte % ROWB) >> 4;
      const int hy = hp / HW_, hx = hp - hy * HW_;
      const int yy = y0 + hy - PADT, xx = hx - PADT;
      const bool ok = hp < HP && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      const unsigned off = ok ? (unsigned)(((((long)r.n * a.H + yy) * a.W + xx) * C + 8 * pc) * 2) : kSatOOB;
      sat_bdma16(rX, st + (d * WS_NW + w) * 1024, off);
    }
  };
  int hp0[WS_MB];
#pragma unroll
  for (int i = 0; i < WS_MB; ++i) hp0[i] = ph * HW_ + i * 16 + fr;

  PRun c;
  c.run = blockIdx.x;
  if (c.run >= a.runs) return;   // workgroup-uniform
  open_run(c);
  PRun s = c;
  stage(s, 0);
  advance(s);
  bool v1 = s.run < a.runs;      // the item after c exists (and is staged)
  if (v1) {
    stage(s, 1);
    advance(s);                  // s: the item two after c
  }
  int st1 = 0, st2 = 0;          // this wave's stores of the previous item and the one before
  int buf = 0, xb = 0;           // ring stage and exchange buffer of this item
  char* xch = smem + NSTG * STG + cg * XCG;
  for (;;) {
    // this wave's DMAs of this item have landed once only younger operations remain: its DMAs of the next item and
    // its stores of the previous one or two items
    const int younger = (v1 ? ndma : 0) + st1 + st2;
    switch (younger) {
#define WP_CASE(k) case k: sat_vm_lds_barrier<k>(); break;
      WP_CASE(3 + 2 * ST) WP_CASE(2 + 2 * ST) WP_CASE(3 + ST) WP_CASE(2 + ST) WP_CASE(3) WP_CASE(2) WP_CASE(2 * ST) WP_CASE(ST)
#undef WP_CASE
      default: sat_vm_lds_barrier<0>(); break;
    }
    const bool v2 = v1 && s.run < a.runs;
    if (v2) stage(s, buf == 0 ? 2 : buf - 1);
    __builtin_amdgcn_sched_barrier(0);
    const char* base = smem + buf * STG;
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) asm volatile("" : "+v"(hp0[i]));
    f32x4 acc[WS_MB];
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto afrag = [&](int i, int ks) {
      const int k = ks * 32 + 8 * fh, tap = k / C, ch = (k % C) >> 3;
      const int hp = hp0[i] + (tap / KK) * HW_ + tap % KK;
      return *(const bf16x8*)(base + hp * ROWB + 16 * ch);
    };
    bf16x8 af[2][WS_MB];
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) af[0][i] = afrag(i, 0);
#pragma unroll
    for (int ks = 0; ks < KSN; ++ks) {
      if (ks + 1 < KSN) {
#pragma unroll
        for (int i = 0; i < WS_MB; ++i) af[(ks + 1) & 1][i] = afrag(i, ks + 1);
      }
#pragma unroll
      for (int i = 0; i < WS_MB; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[ks], af[ks & 1][i], acc[i], 0, 0, 0);
    }
    // the conv launch's output values (bias, ReLU, one bf16 rounding) of pixel 16 i + fr, then the column pool:
    // even fr holds pooled column 8 i + fr / 2
    float cp[WS_MB][4];
    float carry[4];   // pixel 15 of the previous m-block, in lane fr = 0
#pragma unroll
    for (int j = 0; j < 4; ++j) carry[j] = -INFINITY;   // column -1: outside the image
#pragma unroll
    for (int i = 0; i < WS_MB; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = (float)(bf16)apply_act(acc[i][j] + bias4[j], SAT_ACT_RELU);
        const float lft = __shfl(v, (fr + 15) & 15, 16), rgt = __shfl(v, (fr + 1) & 15, 16);
        const float l = fr == 0 ? carry[j] : lft;
        carry[j] = lft;
        cp[i][j] = fmaxf(fmaxf(l, v), rgt);
      }
    }
    const bool even = (fr & 1) == 0;
    const bool emit = c.q >= c.q0;
    if (ph == 1) {
      // row 2q + 1 -> this item's exchange buffer (the values are bf16 already: the conversion is exact)
#pragma unroll
      for (int i = 0; i < WS_MB; ++i) {
        sat_u32x2 cur;
        bf16* cb = (bf16*)&cur;
#pragma unroll
        for (int j = 0; j < 4; ++j) cb[j] = (bf16)cp[i][j];
        if (even) {
          const unsigned addr = (unsigned)(uintptr_t)(sat_lds_char*)(xch + xb * XB + (8 * i + (fr >> 1)) * 32 + 8 * fh);
          asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(cur) : "memory");
        }
      }
    }
    // LDS only: DMAs and stores stay in flight.  After it this item's buffer is written; the other one (the previous
    // item's row 2q + 1 = this item's row 2q - 1) is rewritten only after the next iteration's first barrier, behind
    // the reads below.  At an image top (q = 0) row -1 takes no part; elsewhere the previous item of this workgroup is
    // item q - 1 of the same image (open_run), stored or not.
    sat_lds_barrier();
    int stn = 0;
    if (ph == 0 && emit) {
      sat_u32x2 xr[WS_MB], xp[WS_MB];
#pragma unroll
      for (int i = 0; i < WS_MB; ++i) xr[i] = xp[i] = sat_u32x2{0u, 0u};
      const bool top = c.q == 0;
      if (even) {
#pragma unroll
        for (int i = 0; i < WS_MB; ++i) {
          const unsigned addr = (unsigned)(uintptr_t)(sat_lds_char*)(xch + xb * XB + (8 * i + (fr >> 1)) * 32 + 8 * fh);
          const unsigned addp = (unsigned)(uintptr_t)(sat_lds_char*)(xch + (top ? xb : xb ^ 1) * XB + (8 * i + (fr >> 1)) * 32 + 8 * fh);
          asm volatile("ds_read_b64 %0, %1" : "=v"(xr[i]) : "v"(addr) : "memory");
          asm volatile("ds_read_b64 %0, %1" : "=v"(xp[i]) : "v"(addp) : "memory");
        }
      }
      static_assert(WS_MB == 7, "the wait below names every exchange register");
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(xr[0]), "+v"(xr[1]), "+v"(xr[2]), "+v"(xr[3]), "+v"(xr[4]), "+v"(xr[5]), "+v"(xr[6]),
                     "+v"(xp[0]), "+v"(xp[1]), "+v"(xp[2]), "+v"(xp[3]), "+v"(xp[4]), "+v"(xp[5]), "+v"(xp[6])::"memory");
#pragma unroll
      for (int i = 0; i < WS_MB; ++i) {
        const bf16* xq = (const bf16*)&xr[i];
        const bf16* xo = (const bf16*)&xp[i];
        sat_u32x2 o;
        bf16* ob = (bf16*)&o;
#pragma unroll
        for (int j = 0; j < 4; ++j) ob[j] = (bf16)fmaxf(fmaxf(cp[i][j], (float)xq[j]), (float)xo[j]);
        // odd lanes hold no pooled pixel: their store is dropped through the out-of-range offset, so every lane
        // issues every store (the counted vmcnt)
        const unsigned off = even ? (unsigned)(((((long)c.n * a.ipi + c.q) * PW + 8 * i + (fr >> 1)) * WS_NOUT + 16 * cg + 4 * fh) * 2)
                                  : kSatOOB;
        __builtin_amdgcn_raw_buffer_store_b64(o, rY, (int)off, 0, 0);
      }
      stn = ST;
    }
    if (!v1) break;
    advance(c);
    if (v2) advance(s);
    v1 = v2;
    st2 = st1;
    st1 = stn;
    buf = buf == 2 ? 0 : buf + 1;
    xb ^= 1;
  }
}

__global__ __launch_bounds__(WS_NW * 64, 4) void conv_stem_pool_kernel(PArgs a) {
  const SatStampT0 t0 = sat_stamp_begin(a.st);
  conv_stem_pool_kernel_body(a);
  sat_stamp_end(a.st, t0);
}

template <int KK, int C, int PADT, int TR, int TW, int NSTG>
void launch_ws(int act, dim3 grid, hipStream_t s, const WArgs& a) {
  if (act == SAT_ACT_RELU)
    hipLaunchKernelGGL((conv_ws_kernel<KK, C, PADT, TR, TW, NSTG, SAT_ACT_RELU>), grid, dim3(WS_NW * 64), 0, s, a);
  else
    hipLaunchKernelGGL((conv_ws_kernel<KK, C, PADT, TR, TW, NSTG, SAT_ACT_NONE>), grid, dim3(WS_NW * 64), 0, s, a);
}

}  // namespace

// Returns 1 if the conv was launched by the weight-stationary kernel (3x3 / pad 1 over 64 channels at
// width 56 or 224; the 4x4 / top-left-pad-2 stem over the 16-channel space-to-depth input at width
// 112), 0 otherwise.
int sat_conv3x3_ws_try(const SatGemm& g, hipStream_t s, int* err) {
  *err = 0;
  if (sat_policy().conv3x3_ws == 1) return 0;
  const SatConvGeom& cv = g.conv;
  const bool c3 = cv.C == 64 && cv.KH == 3 && cv.KW == 3 && cv.pad == 1 && (cv.W == 56 || cv.W == 224);
  const bool stem = cv.C == 16 && cv.KH == 4 && cv.KW == 4 && cv.pad == 2 && cv.W == 112;
  if (!(c3 || stem) || g.N != WS_NOUT || cv.stride != 1 || cv.OH != cv.H || cv.OW != cv.W) return 0;
  if (g.dtype != SAT_BF16 || g.c_dtype != SAT_BF16 || g.batch != 1 || g.aux || g.transB || g.add1) return 0;
  if (g.beta != 0.f || g.alpha != 1.f || g.partial_splits > 1) return 0;
  if (g.act != SAT_ACT_NONE && g.act != SAT_ACT_RELU) return 0;
  if (g.ldb != cv.KH * cv.KW * cv.C || g.ldc != WS_NOUT) return 0;
  if (!sat_al16(g.A) || !sat_al16(g.B) || !sat_al16(g.C) || (g.bias && !sat_al16(g.bias))) return 0;
  const int TR = cv.W == 56 ? 4 : 2, TW = cv.W == 56 ? 56 : 112;
  if (cv.H % TR) return 0;
  const long xb = 2L * cv.N * cv.H * cv.W * cv.C, yb = 2L * cv.N * cv.H * cv.W * WS_NOUT;
  if (xb >= (1L << 31) || yb >= (1L << 31)) return 0;
  const int cus = sat_cu_count();
  if (cus == 0) return 0;
  WArgs a{};
  a.x = (const bf16*)g.A; a.w = (const bf16*)g.B; a.bias = g.bias; a.y = (bf16*)g.C;
  a.N = cv.N; a.H = cv.H; a.W = cv.W;
  a.tiles_x = cv.W / TW;
  a.items_per_img = (cv.H / TR) * a.tiles_x;
  a.items = cv.N * a.items_per_img;
  a.x_bytes = (unsigned)xb; a.y_bytes = (unsigned)yb;
  a.st = sat_launch_stamps();
  // the stem variant (72 KB of LDS, 108 VGPRs) fits two workgroups per CU
  const int slots = cus * (stem ? 2 : 1);
  const int grid = a.items < slots ? a.items : slots;
  if (stem) launch_ws<4, 16, 2, 2, 112, 3>(g.act, dim3(grid), s, a);
  else if (cv.W == 56) launch_ws<3, 64, 1, 4, 56, 3>(g.act, dim3(grid), s, a);
  else launch_ws<3, 64, 1, 2, 112, 2>(g.act, dim3(grid), s, a);
  *err = (int)hipGetLastError();
  return 1;
}

// ---- the stem conv + ReLU + 3x3 / stride 2 / pad 1 max pool as one launch ----
namespace {

bool stem_pool_shape(const SatConvGeom& cv, int Cout, int dtype, int relu, int pk, int ps, int pp) {
  if (dtype != SAT_BF16 || !relu || pk != 3 || ps != 2 || pp != 1 || Cout != WS_NOUT) return false;
  if (cv.C != 16 || cv.KH != 4 || cv.KW != 4 || cv.pad != 2 || cv.W != 112 || cv.stride != 1) return false;
  if (cv.OH != cv.H || cv.OW != cv.W || cv.N <= 0 || cv.H <= 0 || cv.H % 2) return false;
  if (2L * cv.N * cv.H * cv.W * cv.C >= (1L << 31) || 2L * cv.N * cv.H * cv.W * WS_NOUT >= (1L << 31)) return false;
  return sat_policy().conv3x3_ws != 1 && sat_cu_count() > 0;
}

}  // namespace

extern "C" int sat_conv_stem_pool_supported(const SatConvGeom* g, int Cout, int dtype, int relu, int pool_k,
                                            int pool_stride, int pool_pad, const SatPolicy* policy) {
  if (!g) return 0;
  SatPolicyScope scope(policy);
  return stem_pool_shape(*g, Cout, dtype, relu, pool_k, pool_stride, pool_pad);
}

extern "C" int sat_conv_stem_pool(const SatConvGeom* g, int Cout, int dtype, const void* x, const void* w,
                                  const float* bias, int relu, int pool_k, int pool_stride, int pool_pad, void* y,
                                  const SatPolicy* policy, void* stream) {
  SAT_REQUIRE(g && x && w && y);
  SatPolicyScope scope(policy);
  // no second path here: the caller issues the conv and the pool where this launch does not apply
  SAT_REQUIRE(stem_pool_shape(*g, Cout, dtype, relu, pool_k, pool_stride, pool_pad));
  SAT_REQUIRE(sat_al16(x) && sat_al16(w) && sat_al16(y) && sat_al16(bias));   // bias: null passes
  const SatConvGeom& cv = *g;
  PArgs a{};
  a.x = (const bf16*)x; a.w = (const bf16*)w; a.bias = bias; a.y = (bf16*)y;
  a.N = cv.N; a.H = cv.H; a.W = cv.W;
  a.ipi = cv.H / 2;
  // runs of whole items inside one image, at least as many as workgroup slots (two per CU) where the images allow it
  const int slots = 2 * sat_cu_count();
  int rpi = sat_cdiv(slots, cv.N);
  if (rpi > a.ipi) rpi = a.ipi;
  a.rl = sat_cdiv(a.ipi, rpi);
  a.rpi = sat_cdiv(a.ipi, a.rl);
  a.runs = cv.N * a.rpi;
  a.x_bytes = (unsigned)(2L * cv.N * cv.H * cv.W * cv.C);
  a.y_bytes = (unsigned)(2L * cv.N * a.ipi * (cv.W / 2) * WS_NOUT);
  a.st = sat_launch_stamps();
  const int grid = a.runs < slots ? a.runs : slots;
  hipLaunchKernelGGL(conv_stem_pool_kernel, dim3(grid), dim3(WS_NW * 64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

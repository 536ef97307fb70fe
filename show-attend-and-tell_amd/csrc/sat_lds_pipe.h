// Device primitives shared by the kernels that stage operands into LDS by DMA and feed MFMA from there
// (convgemm, convpipe, convstream, convblock, conv3x3ws, gemmsplit, skinny).  Internal header; everything here is
// force-inlined and stateless.  Tile shapes, wait counts and SAT_* tuning macros stay with the kernel that owns them.
#pragma once
#include "sat_common.h"

#include <utility>

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void sat_lds_void;
typedef __attribute__((address_space(3))) char sat_lds_char;
typedef __attribute__((address_space(3))) bf16x4 sat_lds_bf16x4;
typedef __attribute__((address_space(1))) const void sat_gbl_void;

// ---- barriers ------------------------------------------------------------------------------------------
// Wait until at most N of this wave's vector-memory operations (LDS-DMAs, loads, stores) are outstanding, then
// barrier.  Always a raw s_barrier, never __syncthreads: its fence would drain every LDS-DMA stage in flight, and
// the rings live on keeping the younger stages (and the last items' stores) pending across the barrier.
//   sat_vm_barrier      vmcnt only.  For kernels with no LDS read pending at the barrier: every fragment read so far
//                       fed an MFMA issued before it, behind the compiler's own lgkmcnt wait (convgemm), or no
//                       stage is ever refilled (skinny's head_out_lds_kernel).
//   sat_vm_lds_barrier  also lgkmcnt(0).  For kernels that request fragments ahead of their use or read LDS in asm
//                       the compiler does not track: a stage may be refilled after the barrier only because every
//                       wave's reads of it retired before it (convpipe, convstream, convblock, conv3x3ws, gemmsplit).
//   sat_lds_barrier     lgkmcnt(0) only: orders LDS writes and reads between waves while DMAs and stores stay in flight.
// Which flavour a kernel uses is part of its correctness argument; do not swap one for another without redoing it.
template <int N>
__device__ __forceinline__ void sat_vm_barrier() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void sat_vm_lds_barrier() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
__device__ __forceinline__ void sat_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- LDS-DMA: 16 B per lane, one wave instruction = 1 KiB of lane-linear LDS starting at `lds` --------------
__device__ __forceinline__ void sat_dma16(const void* src, char* lds) {
  __builtin_amdgcn_global_load_lds((sat_gbl_void*)src, (sat_lds_void*)lds, 16, 0, 0);
}
// through a raw buffer resource: an out-of-range offset (kSatOOB) lands zeros in LDS, so padding taps and rows past
// M or N need one v_cndmask on a 32-bit offset instead of 64-bit address arithmetic and a zero line
__device__ __forceinline__ void sat_bdma16(__amdgpu_buffer_rsrc_t r, char* lds, unsigned voff, unsigned soff = 0) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (sat_lds_void*)lds, 16, (int)voff, (int)soff, 0, 0);
}
// select the source of a global-form DMA without control flow (v_cndmask on the address, one DMA per lane); z is
// the zero line (sat_zero_line(), sat_common.h)
__device__ __forceinline__ const void* sat_sel(bool ok, const void* p, const void* z) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)z;
  return (const void*)(ok ? a : b);
}

// ---- k-major ("transposed") operand tile ---------------------------------------------------------------------
// 64 k-rows x 128 elements = 256-B rows, 16-B chunk ch of row r stored at slot ch ^ sat_swz256(r)
// (cdna_hip_programming.md T10, image (b)): conflict-free for ds_read_b64_tr_b16 fragment reads.
__device__ __forceinline__ int sat_swz256(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }
// MFMA 16x16x32 operand fragment (8 consecutive k of column xt + lane & 15) from a k-major tile: two transposing
// reads of 4 k-rows x 16 columns each
__device__ __forceinline__ bf16x8 sat_frag_kmajor(const char* tile, int kbase, int xt, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const int ch = (xt >> 3) + (p >> 1);
  const int r0 = kbase + 8 * g + q, r1 = r0 + 4;
  const char* a0 = tile + r0 * 256 + 16 * (ch ^ sat_swz256(r0)) + 8 * (p & 1);
  const char* a1 = tile + r1 * 256 + 16 * (ch ^ sat_swz256(r1)) + 8 * (p & 1);
  const bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((sat_lds_bf16x4*)(uintptr_t)(const void*)a0);
  const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((sat_lds_bf16x4*)(uintptr_t)(const void*)a1);
  bf16x8 r;
  r[0] = v0[0]; r[1] = v0[1]; r[2] = v0[2]; r[3] = v0[3];
  r[4] = v1[0]; r[5] = v1[1]; r[6] = v1[2]; r[7] = v1[3];
  return r;
}

// ---- XCD-aware tile order (cdna_hip_programming.md T1, bijective form) ------------------------------------------
// Dispatch round-robins consecutive workgroups over the 8 XCDs; this gives each XCD a contiguous run of the nwg
// row-major tiles, so the workgroups that share an operand panel share one L2.
__device__ __forceinline__ int sat_xcd_tile(int tile, int nwg) {
  const int q = nwg / 8, r = nwg % 8, x = tile % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + tile / 8;
}

// ---- compile-time loop: f(std::integral_constant<int, T>) for T = 0 .. N-1 (register arrays indexed by T stay
// static, every wait count is a literal) ---------------------------------------------------------------------------
template <typename F, int... Ts>
__device__ __forceinline__ void sat_static_for_impl(F&& f, std::integer_sequence<int, Ts...>) {
  (f(std::integral_constant<int, Ts>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sat_static_for(F&& f) {
  sat_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// Row gather / scatter between a large device-resident table and a batch (the feature cache).
//
//   gather :  out[i, :]        = table[idx[i], :]     i < n   (an index outside [0, n_rows): a zero row)
//   scatter:  table[idx[i], :] = src[i, :]            i < n   (an index outside [0, n_rows): the row is skipped)
//
// A table is tens of GB, so every address is a 64-bit pointer sum: no buffer resource (whose offsets and record
// count are 32-bit) anywhere on this path.  The work item is one span of one row, and the grid grows with n x the
// spans of a row: a row is cut into equal spans of at most kUnroll x 256 vectors, and into more, shorter ones while the
// launch has fewer than two workgroups per CU (128 rows of 200 KB: 4 spans of 3136 vectors each, 512 workgroups;
// fewer, longer spans measured faster than 1664 workgroups of a quarter the size).  Every lane issues all
// its loads of the span before the first store.  Rows move as 16-B vectors when the row bytes and both base pointers
// are 16-B aligned (then every row of both tensors is), else element by element.  The indices are read on the device
// (a captured launch follows a rewritten index buffer), nothing is memset, and a bad row adds 1 to *n_bad with a
// plain atomicAdd.
#include "sat_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 16;
constexpr long kMaxSpan = (long)kThreads * kUnroll;   // vectors of one work item at the most
constexpr long kMinSpan = kThreads;                   // ... and, when a row is cut finer to fill the chip, at the least
constexpr long kMaxGrid = 1L << 16;                   // past this the workgroups stride over the work items

template <typename V, bool SCATTER>
__global__ __launch_bounds__(kThreads) void rows_kernel(const V* __restrict__ src, V* __restrict__ dst,
                                                        const int64_t* __restrict__ idx, long n_rows, long row_v,
                                                        long spans_per_row, long span, long total,
                                                        int32_t* __restrict__ n_bad) {
  for (long c = blockIdx.x; c < total; c += gridDim.x) {   // uniform
    const long i = c / spans_per_row;
    const long sp = c - i * spans_per_row;
    const long r = idx[i];
    const bool ok = r >= 0 && r < n_rows;   // uniform
    if (!ok) {
      if (sp == 0 && threadIdx.x == 0 && n_bad) atomicAdd(n_bad, 1);
      if (SCATTER) continue;
    }
    const V* s = src + (SCATTER ? i : (ok ? r : 0)) * row_v;
    V* d = dst + (SCATTER ? r : i) * row_v;
    const long j0 = sp * span + threadIdx.x;
    const long end = (sp + 1) * span < row_v ? (sp + 1) * span : row_v;   // span <= kMaxSpan: kUnroll steps cover it
    V v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long j = j0 + (long)u * kThreads;
      v[u] = V{};
      if (ok && j < end) v[u] = s[j];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long j = j0 + (long)u * kThreads;
      if (j < end) d[j] = v[u];
    }
  }
}

template <typename V, bool SCATTER>
int launch(const void* src, void* dst, const int64_t* idx, long n, long n_rows, long row_v, int32_t* n_bad,
           hipStream_t s) {
  const long cus = sat_cu_count() > 0 ? sat_cu_count() : 256;
  long spans = (row_v + kMaxSpan - 1) / kMaxSpan;   // the fewest a row needs
  const long fill = (2 * cus + n - 1) / n;          // ... more while that leaves CUs without two workgroups
  const long finest = (row_v + kMinSpan - 1) / kMinSpan;
  if (spans < fill) spans = fill < finest ? fill : finest;
  const long span = (row_v + spans - 1) / spans;
  spans = (row_v + span - 1) / span;                // no empty span
  const long total = n * spans;
  const long grid = total < kMaxGrid ? total : kMaxGrid;
  hipLaunchKernelGGL((rows_kernel<V, SCATTER>), dim3((unsigned)grid), dim3(kThreads), 0, s, (const V*)src, (V*)dst,
                     idx, n_rows, row_v, spans, span, total, n_bad);
  return (int)hipGetLastError();
}

template <bool SCATTER>
int dispatch(const void* src, void* dst, const int64_t* idx, long n, long n_rows, long row_elems, int dtype,
             int32_t* n_bad, hipStream_t s) {
  const long esize = dtype == SAT_BF16 ? 2 : 4;
  const long row_bytes = row_elems * esize;
  if (row_bytes % 16 == 0 && sat_al16(src) && sat_al16(dst))
    return launch<sat_u32x4, SCATTER>(src, dst, idx, n, n_rows, row_bytes / 16, n_bad, s);
  if (esize == 2) return launch<uint16_t, SCATTER>(src, dst, idx, n, n_rows, row_elems, n_bad, s);
  return launch<uint32_t, SCATTER>(src, dst, idx, n, n_rows, row_elems, n_bad, s);
}

}  // namespace

extern "C" int sat_rows_gather(const void* table, int64_t n_rows, int64_t row_elems, int dtype, const int64_t* idx,
                               int n, void* out, int32_t* n_bad, void* stream) {
  SAT_REQUIRE(table && idx && out && n >= 0 && n_rows > 0 && row_elems > 0);
  SAT_REQUIRE(dtype == SAT_F32 || dtype == SAT_BF16);
  if (n == 0) return 0;
  return dispatch<false>(table, out, idx, n, n_rows, row_elems, dtype, n_bad, (hipStream_t)stream);
}

extern "C" int sat_rows_scatter(const void* src, int n, int64_t row_elems, int dtype, const int64_t* idx, void* table,
                                int64_t n_rows, int32_t* n_bad, void* stream) {
  SAT_REQUIRE(src && idx && table && n >= 0 && n_rows > 0 && row_elems > 0);
  SAT_REQUIRE(dtype == SAT_F32 || dtype == SAT_BF16);
  if (n == 0) return 0;
  return dispatch<true>(src, table, idx, n, n_rows, row_elems, dtype, n_bad, (hipStream_t)stream);
}

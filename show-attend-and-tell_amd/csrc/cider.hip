// CIDEr-D on the device: the sentence reward of self-critical sequence training without a host round trip
// (DESIGN 4.19).  The arithmetic is sat_amd/cider.py's (CiderD.score_one):
//
//   weight(g) = tf(g) * idf(g),  idf(g) = log N - log max(1, df(g))     n-grams g of n = 1..4 words
//   score     = 10 / (4 R) * sum_{refs r} exp(-(L_h - L_r)^2 / 72) * sum_n dot_n / (|h_n| |r_n|)
//   dot_n     = sum_{g in h and r} min(w_h(g), w_r(g)) * w_r(g)         a term with either norm 0 is skipped
//
// The corpus is resident: the stripped reference words [n_refs, ref_stride] with their lengths, a CSR from image to
// references, the references' norms [n_refs, 4] and an open-addressed hash table from n-gram to idf.
//
// The table.  One slot is 16 bytes: the 96-bit key and the fp32 idf.  The key holds the whole n-gram and its n
// (word 0 = n << 20 | id0, so no key has word 0 == 0 and an empty slot is word 0 == 0; ids are below 2^20), so a hash
// collision costs a probe and never a value.  The inserted keys are unique: an inserter claims a slot with one atomicCAS
// on word 0 and writes the other three words with plain stores; it never looks at another inserter's slot beyond
// "word 0 is taken".  Lookups happen in later launches.  Every probe loop ends after `slots` probes.
//
// The scorer.  One wave per hypothesis row (one 64-thread workgroup).  Lane t reads token t; a ballot of the end ids
// gives the cut, a ballot of the kept lanes and a prefix count give every word its place, so an n-gram spans a dropped
// token as strip_ids makes it.  Lane i owns the n-gram that starts at word i: its tf and whether it is the first of its
// kind come from comparing against the row's other positions in LDS (L <= 64), the reference's count the same way
// against the reference's words.  Sums run over the 64 lanes in a fixed butterfly, in fp64 from fp32 weights.
#include "sat_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxWords = 64;          // words of a hypothesis / a reference at the most
constexpr int kNMax = 4;
constexpr int kIdLimit = 1 << 20;
constexpr int kLdsWords = kMaxWords + kNMax;   // an n-gram read at the last word stays inside the array

struct Key {
  uint32_t a, b, c;
};

// ids below 2^20; the ids past n are not part of the key
__device__ __forceinline__ Key pack_key(int n, const int* w) {
  const uint32_t i0 = (uint32_t)w[0], i1 = n > 1 ? (uint32_t)w[1] : 0u, i2 = n > 2 ? (uint32_t)w[2] : 0u,
                 i3 = n > 3 ? (uint32_t)w[3] : 0u;
  return Key{((uint32_t)n << 20) | i0, i1 | ((i2 & 0xfffu) << 20), (i2 >> 12) | (i3 << 8)};
}

__device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t hash_key(Key k) {
  return mix32(k.a ^ mix32(k.b ^ mix32(k.c ^ 0x9e3779b9u)));
}

// the stored idf of k, or `absent` (log N: df 0) when k is not in the table; at most `slots` probes
__device__ float table_lookup(const uint4* __restrict__ table, uint32_t slots, Key k, float absent) {
  uint32_t s = hash_key(k) % slots;
  for (uint32_t probe = 0; probe < slots; ++probe) {
    const uint4 e = table[s];
    if (e.x == 0u) return absent;
    if (e.x == k.a && e.y == k.b && e.z == k.c) return __uint_as_float(e.w);
    s = s + 1 == slots ? 0u : s + 1;
  }
  return absent;
}

__global__ __launch_bounds__(256) void insert_kernel(uint32_t* __restrict__ table, uint32_t slots,
                                                     const uint32_t* __restrict__ keys,
                                                     const float* __restrict__ values, long n,
                                                     int32_t* __restrict__ n_bad) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Key k{keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]};
  bool placed = false;
  if (k.a != 0u) {   // word 0 == 0 marks an empty slot: such a key cannot be stored
    uint32_t s = hash_key(k) % slots;
    for (uint32_t probe = 0; probe < slots && !placed; ++probe) {
      uint32_t* e = table + 4 * (size_t)s;
      if (atomicCAS(e, 0u, k.a) == 0u) {
        e[1] = k.b;
        e[2] = k.c;
        e[3] = __float_as_uint(values[i]);
        placed = true;
      }
      s = s + 1 == slots ? 0u : s + 1;
    }
  }
  if (!placed && n_bad) atomicAdd(n_bad, 1);
}

__global__ __launch_bounds__(256) void lookup_kernel(const uint4* __restrict__ table, uint32_t slots, float log_n,
                                                     const uint32_t* __restrict__ keys, long n,
                                                     float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = table_lookup(table, slots, Key{keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]}, log_n);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ bool same_gram(const int* a, const int* b, int n) {
  bool eq = a[0] == b[0];
  if (n > 1) eq = eq && a[1] == b[1];
  if (n > 2) eq = eq && a[2] == b[2];
  if (n > 3) eq = eq && a[3] == b[3];
  return eq;
}

// how often the n-gram at g occurs among the n-grams of words[0 .. len)
__device__ __forceinline__ int count_gram(const int* words, int len, const int* g, int n) {
  int c = 0;
  for (int j = 0; j + n <= len; ++j) c += same_gram(words + j, g, n) ? 1 : 0;   // j uniform: an LDS broadcast
  return c;
}

// The lane's n-gram (the one starting at word `lane` of words[0 .. len), in LDS): its count in the sentence when the
// lane holds the sentence's first occurrence of it, else 0; *idf = its idf then.  An id outside [0, 2^20) is in no
// reference: df 0.
__device__ __forceinline__ int own_gram(const int* words, int len, int lane, int n, const uint4* table,
                                        uint32_t slots, float log_n, float* idf) {
  *idf = 0.f;
  if (lane + n > len) return 0;
  const int* g = words + lane;
  int tf = 0;
  bool first = true;
  for (int j = 0; j + n <= len; ++j) {
    const bool eq = same_gram(words + j, g, n);
    tf += eq ? 1 : 0;
    first = first && !(eq && j < lane);
  }
  if (!first) return 0;
  bool in_range = true;
  for (int q = 0; q < n; ++q) in_range = in_range && g[q] >= 0 && g[q] < kIdLimit;
  *idf = in_range ? table_lookup(table, slots, pack_key(n, g), log_n) : log_n;
  return tf;
}

// one wave per reference: norm[r, n-1] = sqrt(sum over its distinct n-grams of (tf idf)^2)
__global__ __launch_bounds__(kWave) void ref_norms_kernel(const uint4* __restrict__ table, uint32_t slots, float log_n,
                                                          const int32_t* __restrict__ ref_words,
                                                          const int32_t* __restrict__ ref_len, int ref_stride,
                                                          float* __restrict__ ref_norm) {
  __shared__ int words[kLdsWords];
  const int r = blockIdx.x, lane = threadIdx.x;
  int len = ref_len[r];
  len = len < 0 ? 0 : (len > ref_stride ? ref_stride : len);   // ref_stride <= kMaxWords
  words[lane] = lane < len ? ref_words[(long)r * ref_stride + lane] : -1;
  if (lane < kNMax) words[kMaxWords + lane] = -1;
  __syncthreads();
#pragma unroll
  for (int n = 1; n <= kNMax; ++n) {
    float idf;
    const int tf = own_gram(words, len, lane, n, table, slots, log_n, &idf);
    const double w = (double)((float)tf * idf);
    const double s = wave_sum_f64(w * w);
    if (lane == 0) ref_norm[(long)r * kNMax + n - 1] = (float)sqrt(s);
  }
}

__global__ __launch_bounds__(kWave) void score_kernel(const uint4* __restrict__ table, uint32_t slots, float log_n,
                                                      const int32_t* __restrict__ ref_words,
                                                      const int32_t* __restrict__ ref_len,
                                                      const float* __restrict__ ref_norm, int n_refs, int ref_stride,
                                                      const int32_t* __restrict__ img_ref_begin, int n_images,
                                                      const int32_t* __restrict__ tokens,
                                                      const int64_t* __restrict__ image, int T1, int start_id,
                                                      int end_id, int pad_id, float* __restrict__ out,
                                                      int32_t* __restrict__ n_bad) {
  __shared__ int hyp[kLdsWords];
  __shared__ int ref[kLdsWords];
  const int row = blockIdx.x, lane = threadIdx.x;

  // ---- strip: drop start / pad ids wherever they stand, cut before the first end id
  const bool have = lane < T1;
  const int tok = have ? tokens[(long)row * T1 + lane] : 0;
  const unsigned long long ends = __ballot(have && tok == end_id);
  const int cut = ends ? __ffsll((long long)ends) - 1 : T1;
  const bool keep = have && lane < cut && tok != start_id && tok != pad_id;
  const unsigned long long kept = __ballot(keep);
  const int len = __popcll(kept);
  const int pos = __popcll(kept & ((1ull << lane) - 1ull));
  hyp[lane] = -1;
  if (lane < kNMax) hyp[kMaxWords + lane] = -1;
  __syncthreads();
  if (keep) hyp[pos] = tok;
  __syncthreads();

  const long img = image[row];
  const bool img_ok = img >= 0 && img < n_images;   // uniform
  if (!img_ok) {
    if (lane == 0) {
      out[row] = 0.f;
      if (n_bad) atomicAdd(n_bad, 1);
    }
    return;
  }
  int r0 = img_ref_begin[img], r1 = img_ref_begin[img + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > n_refs ? n_refs : r1;
  if (len == 0 || r1 <= r0) {   // an empty hypothesis, an image without references
    if (lane == 0) out[row] = 0.f;
    return;
  }

  // ---- the hypothesis' vector: per n the lane's weight (0 unless it holds a first occurrence) and the norm
  float idf_h[kNMax], w_h[kNMax];
  double norm_h[kNMax];
#pragma unroll
  for (int n = 1; n <= kNMax; ++n) {
    const int tf = own_gram(hyp, len, lane, n, table, slots, log_n, &idf_h[n - 1]);
    w_h[n - 1] = (float)tf * idf_h[n - 1];
    const double w = (double)w_h[n - 1];
    norm_h[n - 1] = sqrt(wave_sum_f64(w * w));
  }

  // ---- against every reference of the image, in order
  double total = 0.0;
  for (int r = r0; r < r1; ++r) {   // uniform
    int rl = ref_len[r];
    rl = rl < 0 ? 0 : (rl > ref_stride ? ref_stride : rl);
    __syncthreads();   // the previous reference's readers are done
    ref[lane] = lane < rl ? ref_words[(long)r * ref_stride + lane] : -1;
    if (lane < kNMax) ref[kMaxWords + lane] = -1;
    __syncthreads();
    const double dl = (double)(len - rl);
    const double penalty = exp(-(dl * dl) / 72.0);   // sigma = 6
#pragma unroll
    for (int n = 1; n <= kNMax; ++n) {
      const double nr = (double)ref_norm[(long)r * kNMax + n - 1];
      if (norm_h[n - 1] == 0.0 || nr == 0.0) continue;   // uniform
      double term = 0.0;
      if (w_h[n - 1] != 0.f) {   // a first occurrence of nonzero weight: an n-gram of weight 0 adds 0 on the host too
        const int c = count_gram(ref, rl, hyp + lane, n);
        const float w_r = (float)c * idf_h[n - 1];
        term = (double)fminf(w_h[n - 1], w_r) * (double)w_r;
      }
      const double dot = wave_sum_f64(term);
      total += dot / (norm_h[n - 1] * nr) * penalty;
    }
  }
  if (lane == 0) out[row] = (float)(10.0 * total / (double)(kNMax * (r1 - r0)));
}

bool slots_ok(int64_t slots) { return slots >= 2 && slots < (1LL << 31); }

}  // namespace

extern "C" int sat_cider_table_insert(uint32_t* table, int64_t slots, const uint32_t* keys, const float* values,
                                      int64_t n, int32_t* n_bad, void* stream) {
  SAT_REQUIRE(table && slots_ok(slots) && n >= 0 && n < (1LL << 31) && sat_al16(table));
  if (n == 0) return 0;
  SAT_REQUIRE(keys && values);
  hipLaunchKernelGGL(insert_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, table,
                     (uint32_t)slots, keys, values, (long)n, n_bad);
  return (int)hipGetLastError();
}

extern "C" int sat_cider_lookup(const uint32_t* table, int64_t slots, float log_n, const uint32_t* keys, int64_t n,
                                float* out, void* stream) {
  SAT_REQUIRE(table && slots_ok(slots) && n >= 0 && n < (1LL << 31) && sat_al16(table));
  if (n == 0) return 0;
  SAT_REQUIRE(keys && out);
  hipLaunchKernelGGL(lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint4*)table, (uint32_t)slots, log_n, keys, (long)n, out);
  return (int)hipGetLastError();
}

extern "C" int sat_cider_ref_norms(const uint32_t* table, int64_t slots, float log_n, const int32_t* ref_words,
                                   const int32_t* ref_len, int n_refs, int ref_stride, float* ref_norm, void* stream) {
  SAT_REQUIRE(table && slots_ok(slots) && sat_al16(table) && n_refs >= 0);
  SAT_REQUIRE(ref_stride >= 1 && ref_stride <= kMaxWords);
  if (n_refs == 0) return 0;
  SAT_REQUIRE(ref_words && ref_len && ref_norm);
  hipLaunchKernelGGL(ref_norms_kernel, dim3((unsigned)n_refs), dim3(kWave), 0, (hipStream_t)stream,
                     (const uint4*)table, (uint32_t)slots, log_n, ref_words, ref_len, ref_stride, ref_norm);
  return (int)hipGetLastError();
}

extern "C" int sat_cider_score(const uint32_t* table, int64_t slots, float log_n, const int32_t* ref_words,
                               const int32_t* ref_len, const float* ref_norm, int n_refs, int ref_stride,
                               const int32_t* img_ref_begin, int n_images, const int32_t* tokens,
                               const int64_t* image, int n, int T1, int start_id, int end_id, int pad_id, float* out,
                               int32_t* n_bad, void* stream) {
  SAT_REQUIRE(table && slots_ok(slots) && sat_al16(table) && n_refs >= 0 && n_images >= 0 && n >= 0);
  SAT_REQUIRE(ref_stride >= 1 && ref_stride <= kMaxWords && T1 >= 1 && T1 <= kMaxWords);
  SAT_REQUIRE(img_ref_begin && (n_refs == 0 || (ref_words && ref_len && ref_norm)));
  if (n == 0) return 0;
  SAT_REQUIRE(tokens && image && out);
  hipLaunchKernelGGL(score_kernel, dim3((unsigned)n), dim3(kWave), 0, (hipStream_t)stream, (const uint4*)table,
                     (uint32_t)slots, log_n, ref_words, ref_len, ref_norm, n_refs, ref_stride, img_ref_begin, n_images,
                     tokens, image, T1, start_id, end_id, pad_id, out, n_bad);
  return (int)hipGetLastError();
}

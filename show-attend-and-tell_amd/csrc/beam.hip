// Beam-search captioning (decoder.py:160-269, Decoder.caption) on the HIP decoder step.
//
// The reference runs one LSTM step for the k live beams per iteration, adds each beam's running
// score to its raw logits, takes the top-k of the flattened [k, V] scores, appends the words,
// retires beams that emitted an end token and compacts the survivors' (h, c, features) by their
// parent index.  Here every tensor step runs on the GPU (one fused kernel sequence per
// iteration, all rows of the live beam batched into each launch) and the host keeps only the
// per-beam word/alpha histories the reference keeps in Python lists: one small D2H of the k
// winners (+ their alpha rows) and one H2D of the compaction indices per iteration.
//
// Device state is sized for the initial beam width; each iteration ping-pongs the gathered
// per-beam feature / W·a rows so the compaction never reads what it writes.
//
// The second half of the file is the batched search (sat_decoder_beam_search_batch): N images x R beams per launch
// on the same decoder step, with the selection, retirement, histories and backtrack on the device.
#include <math.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "sat_common.h"
#include "sat_internal.h"

namespace {

struct BeamWS {
  void *feat[2], *Ws[2], *h_t, *h_new, *emb_t, *ctx_t, *gated_t, *comb_t, *mean_t;
  float *c, *c_new, *h_f32, *xg, *hg, *gctx, *gates, *ctx, *gate, *alpha, *fh, *fz, *logits, *top_val, *mean_f,
      *hc0;
  int32_t *upl, *top_idx;  // upl = [gather idx k | tokens k | scores k (float bits)]
};

// nbuf: copies of the per-row feature / W·a rows (2 = the single-image search's ping-pong, 1 = the batched search,
// whose rows never move)
size_t beam_carve(const SatDecoderDims& d, int R, char* base, BeamWS* w, int nbuf = 2) {
  const size_t L = d.L, D = d.D, E = d.E, V = d.V, HG = 5 * E + D;
  const size_t ts = d.dtype == SAT_BF16 ? 2 : 4, f = 4;
  size_t off = 0;
  auto take = [&](auto*& p, size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    p = base ? (std::remove_reference_t<decltype(p)>)(base + off) : nullptr;
    off += bytes;
  };
  w->feat[1] = w->Ws[1] = nullptr;
  for (int i = 0; i < nbuf; ++i) { take(w->feat[i], R * L * D * ts); take(w->Ws[i], R * L * E * ts); }
  take(w->h_t, R * E * ts); take(w->h_new, R * E * ts); take(w->emb_t, R * E * ts);
  take(w->ctx_t, R * D * ts); take(w->gated_t, R * D * ts); take(w->comb_t, R * E * ts);
  take(w->mean_t, R * D * ts);
  take(w->c, R * E * f); take(w->c_new, R * E * f); take(w->h_f32, R * E * f);
  take(w->xg, R * 4 * E * f); take(w->hg, R * HG * f); take(w->gctx, R * 4 * E * f); take(w->gates, R * 4 * E * f);
  take(w->ctx, R * D * f); take(w->gate, R * D * f); take(w->alpha, R * L * f);
  take(w->fh, R * E * f); take(w->fz, R * E * f); take(w->logits, R * V * f);
  take(w->top_val, R * f); take(w->mean_f, R * D * f); take(w->hc0, R * 2 * E * f);
  take(w->upl, 3 * R * 4); take(w->top_idx, R * 4);
  return off + 256;
}

// ---- top-k of (logits[r, v] + score[r]) over r < rows, v < V --------------------------------
// torch.topk(largest=True, sorted=True) over the flattened scores (decoder.py:204-209).  K <= 64
// passes of one block-wide arg-max each; pass j takes the best element strictly after pass j-1's
// winner in (value desc, index asc) order, so no element is marked or copied.  Ties are broken
// by the lower flat index (torch leaves the order of equal values unspecified).
constexpr int TOPK_THREADS = 1024;

__device__ __forceinline__ bool tk_better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// candidate (v, i) against this pass's best (bv, bi); only candidates after the previous winner (pv, pi) count
__device__ __forceinline__ void tk_consider(float v, int i, float pv, int pi, float& bv, int& bi) {
  const bool after = v < pv || (v == pv && i > pi);
  if (after && tk_better(v, i, bv, bi)) { bv = v; bi = i; }
}

// The K passes over the candidates scan(pv, pi, bv, bi) offers to tk_consider, each thread its share.
// top_val / top_idx [K]: global or shared memory; complete (for every thread of the block) on return
template <class Scan>
__device__ __forceinline__ void block_topk_passes(int K, Scan scan, float* top_val, int32_t* top_idx) {
  __shared__ float sv[TOPK_THREADS / 64];
  __shared__ int si[TOPK_THREADS / 64];
  __shared__ float pv_s;
  __shared__ int pi_s;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < K; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    scan(pv, pi, bv, bi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { sv[wid] = bv; si[wid] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float b = sv[0];
      int ib = si[0];
      for (int w = 1; w < TOPK_THREADS / 64; ++w)
        if (tk_better(sv[w], si[w], b, ib)) { b = sv[w]; ib = si[w]; }
      top_val[j] = b;
      top_idx[j] = ib;
      pv_s = b;
      pi_s = ib;
    }
    __syncthreads();
    pv = pv_s;
    pi = pi_s;
  }
}

// candidates: logits[r, c] + score[r] with flat index idx0 + r * V + c
__device__ __forceinline__ void block_topk(const float* __restrict__ logits, long ld, const float* __restrict__ score,
                                           int rows, int V, int K, int idx0, float* top_val, int32_t* top_idx) {
  block_topk_passes(K, [=](float pv, int pi, float& bv, int& bi) {
    for (int r = 0; r < rows; ++r) {   // row by row: no division per element (the order is total, so any visit order)
      const float* row = logits + (long)r * ld;
      const float sc = score ? score[r] : 0.f;
      const int i0 = idx0 + r * V;
#pragma unroll 4
      for (int c = threadIdx.x; c < V; c += TOPK_THREADS) tk_consider(row[c] + sc, i0 + c, pv, pi, bv, bi);
    }
  }, top_val, top_idx);
}

__global__ void __launch_bounds__(TOPK_THREADS) beam_topk_kernel(const float* __restrict__ logits, long ld,
                                                                 const float* __restrict__ score, int rows, int V,
                                                                 int K, float* top_val, int32_t* top_idx) {
  block_topk(logits, ld, score, rows, V, K, 0, top_val, top_idx);
}

// ---- compaction: dst_q[i] = src_q[idx[i]] for up to 6 row tensors (16-byte rows) -----------
struct GatherSet {
  const void* src[6];
  void* dst[6];
  long row_bytes[6];
  int n;
};

__global__ void beam_gather_kernel(GatherSet g, const int32_t* __restrict__ idx) {
  const int q = blockIdx.y;
  if (q >= g.n) return;
  const long rb = g.row_bytes[q] >> 4;
  const uint4* s = (const uint4*)g.src[q] + (long)idx[blockIdx.x] * rb;
  uint4* d = (uint4*)g.dst[q] + (long)blockIdx.x * rb;
  for (long i = threadIdx.x; i < rb; i += blockDim.x) d[i] = s[i];
}

struct BeamCtx {
  SatDecoderDims d;
  SatDecoderLayout lay;
  const float* P;
  const void* LP;
  const void* W(int64_t off) const {
    return d.dtype == SAT_BF16 ? (const void*)((const bf16*)LP + off) : (const void*)(P + off);
  }
  const float* F(int64_t off) const { return off < 0 ? nullptr : P + off; }
};

int lin(const BeamCtx& c, int rows, int N, int K, const void* x, long ldx, const void* w, long ldw, const float* bias,
        void* y, long ldy, int act, hipStream_t s, void* aux = nullptr, long ld_aux = 0, int aux_dtype = SAT_F32,
        int y_dtype = SAT_F32) {
  SatGemm g;
  g.M = rows; g.N = N; g.K = K; g.dtype = c.d.dtype;
  g.A = x; g.lda = ldx; g.B = w; g.ldb = ldw;
  g.C = y; g.ldc = ldy; g.c_dtype = y_dtype; g.bias = bias; g.act = act;
  g.aux = aux; g.ld_aux = ld_aux; g.aux_dtype = aux_dtype;
  return sat_gemm_launch(g, s);
}

__global__ void ado_sum_kernel(const float* fh, const float* fz, const void* emb, long n, int dt, void* out) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    st_from_f32(out, i, dt, fh[i] + fz[i] + ld_as_f32(emb, i, dt));
}

// One decoder step for k live beams: decoder.py:183-204 (no dropout in caption()).  Leaves the
// raw logits in w.logits [k, V] fp32, alpha rows in w.alpha, the new state in h_new / c_new.
// `feat` / `Ws` are the current per-beam rows, `tok` the k fed words, `alpha` where the k alpha rows go.  fixed_ctx
// (no attention only): w.ctx_t already holds the rows' mean features and the caller filled `alpha`.
int beam_step(const BeamCtx& c, const BeamWS& w, int k, const void* feat, const void* Ws, const int32_t* tok,
              float* alpha, bool fixed_ctx, hipStream_t s) {
  const SatDecoderDims& d = c.d;
  const int L = d.L, D = d.D, E = d.E, V = d.V, HG = 5 * E + D;
  const SatDecoderLayout& lay = c.lay;
  // embedding of the fed words (decoder.py:183) and its half of the LSTM input GEMM (+ b_ih)
  SAT_CHECK((hipError_t)sat_embed_gather(c.F(lay.embedding), tok, k, 1, 1, E, d.dtype, w.emb_t, E, s));
  SAT_CHECK((hipError_t)lin(c, k, 4 * E, E, w.emb_t, E, c.W(lay.wih), E + D, c.F(lay.bih), w.xg, 4 * E,
                            SAT_ACT_NONE, s));
  if (d.attention) {
    // [U h + b | f_beta h + b | W_hh h + b_hh] (attention.py:15, decoder.py:187, LSTMCell)
    SAT_CHECK((hipError_t)lin(c, k, HG, E, w.h_t, E, c.W(lay.hcat_w), E, c.F(lay.hcat_b), w.hg, HG, SAT_ACT_NONE, s));
    AttnFwdArgs a{};
    a.B = k; a.L = L; a.D = D; a.E = E; a.dtype = d.dtype;
    a.Ws = Ws; a.uh = w.hg; a.uh_ld = HG; a.v_w = c.F(lay.v_w); a.v_b = c.F(lay.v_b); a.a = feat;
    a.gate_pre = w.hg + E; a.gate_ld = HG;
    a.hg_splits = 1; a.hg_split_stride = 0;
    a.alpha = alpha; a.alpha_ld = L;
    a.ctx = w.ctx; a.ctx_ld = D;
    a.ctx_t = w.ctx_t; a.ctx_t_ld = D;
    a.gate = w.gate; a.gate_out_ld = D;
    a.gated = w.gated_t; a.gated_ld = D;
    SAT_CHECK((hipError_t)sat_attention_fwd_launch(a, s));
    SAT_CHECK((hipError_t)lin(c, k, 4 * E, D, w.gated_t, D, c.W(lay.wih + E), E + D, nullptr, w.gctx, 4 * E,
                              SAT_ACT_NONE, s));
  } else {  // uniform attention over the (gathered) rows: decoder.py:190-194
    if (!fixed_ctx) {
      SAT_CHECK((hipError_t)sat_mean_rows(feat, k, L, D, d.dtype, w.ctx, w.ctx_t, s));
      SAT_CHECK((hipError_t)sat_fill_const(alpha, (long)k * L, 1.0f / (float)L, s));
    }
    SAT_CHECK((hipError_t)lin(c, k, 4 * E, D, w.ctx_t, D, c.W(lay.wih + E), E + D, nullptr, w.gctx, 4 * E,
                              SAT_ACT_NONE, s));
    SAT_CHECK((hipError_t)lin(c, k, 4 * E, E, w.h_t, E, c.W(lay.hcat_w + (long)(E + D) * E), E,
                              c.F(lay.hcat_b + E + D), w.hg + E + D, HG, SAT_ACT_NONE, s));
  }
  LstmFwdArgs l{};
  l.B = k; l.E = E; l.dtype = d.dtype;
  l.hpart = w.hg + E + D; l.hpart_ld = HG;
  l.xpart = w.xg; l.xpart_ld = 4 * E;
  l.cpart = w.gctx; l.cpart_ld = 4 * E;
  l.h_splits = 1; l.c_splits = 1;
  l.c_prev = w.c; l.c_prev_ld = E;
  l.gates = w.gates; l.gates_ld = 4 * E;
  l.c_out = w.c_new; l.c_out_ld = E;
  l.h_out = w.h_f32; l.h_out_ld = E;
  l.h_next_in_t = w.h_new; l.h_next_in_t_ld = E;
  SAT_CHECK((hipError_t)sat_lstm_fwd_launch(l, s));
  if (d.ado) {  // decoder.py:199-201,149-158 (context is the ungated one)
    SAT_CHECK((hipError_t)lin(c, k, E, E, w.h_new, E, c.W(lay.fh_w), E, c.F(lay.fh_b), w.fh, E, SAT_ACT_RELU, s));
    SAT_CHECK((hipError_t)lin(c, k, E, D, w.ctx_t, D, c.W(lay.fz_w), D, c.F(lay.fz_b), w.fz, E, SAT_ACT_RELU, s));
    const long n = (long)k * E;
    hipLaunchKernelGGL(ado_sum_kernel, dim3(sat_cdiv(n, 256)), dim3(256), 0, s, w.fh, w.fz, (const void*)w.emb_t, n,
                       d.dtype, w.comb_t);
    SAT_LAUNCH_CHECK();
    SAT_CHECK((hipError_t)lin(c, k, V, E, w.comb_t, E, c.W(lay.fout_w), E, c.F(lay.fout_b), w.logits, V,
                              SAT_ACT_RELU, s));
  } else {      // decoder.py:203
    SAT_CHECK((hipError_t)lin(c, k, V, E, w.h_new, E, c.W(lay.do_w), E, c.F(lay.do_b), w.logits, V, SAT_ACT_NONE, s));
  }
  return 0;
}

int gather_rows(const GatherSet& g, const int32_t* idx, int k, hipStream_t s) {
  for (int q = 0; q < g.n; ++q)
    if ((g.row_bytes[q] & 15) || (((uintptr_t)g.src[q] | (uintptr_t)g.dst[q]) & 15)) return SAT_ERR_INVALID;
  hipLaunchKernelGGL(beam_gather_kernel, dim3(k, g.n), dim3(256), 0, s, g, idx);
  return (int)hipGetLastError();
}

int check_beam(const SatDecoderDims* d, int beam) {
  if (!d) return SAT_ERR_INVALID;
  if (d->L <= 0 || d->D <= 0 || d->E <= 0 || d->V <= 0 || beam <= 0 || beam > 64) return SAT_ERR_INVALID;
  if (d->dtype != SAT_F32 && d->dtype != SAT_BF16) return SAT_ERR_INVALID;
  if (d->E % 8 != 0 || d->D % 8 != 0 || d->E > 1024 || d->L > 1024) return SAT_ERR_INVALID;
  if ((long)beam * d->V >= 0x7fffffffL) return SAT_ERR_INVALID;
  return 0;
}

}  // namespace

extern "C" size_t sat_decoder_beam_workspace_bytes(const SatDecoderDims* d, int beam_size) {
  if (check_beam(d, beam_size)) return 0;
  BeamWS w;
  return beam_carve(*d, beam_size, nullptr, &w);
}

extern "C" int sat_decoder_beam_search(const SatDecoderDims* dp, const SatDecoderLayout* lay, const float* params,
                                       const void* params_lp, const void* img_features, int beam_size, int max_step,
                                       void* workspace, size_t workspace_bytes, int32_t* out_ids, int* out_len,
                                       float* out_alphas, int* out_alpha_rows, float* out_score, void* stream) {
  SAT_CHECK((hipError_t)check_beam(dp, beam_size));
  SAT_REQUIRE(lay && params && img_features && workspace && out_ids && out_len && out_alphas && out_alpha_rows &&
              out_score && max_step >= 0);
  SAT_REQUIRE(dp->dtype == SAT_F32 || params_lp);
  SAT_REQUIRE(beam_size <= max_step + 2);  // out_alphas holds (max_step + 2) * L floats
  SatPolicyScope scope(dp->policy);
  SatStampScope no_stamps(nullptr, 0);
  const SatDecoderDims& d = *dp;
  const int R = beam_size, L = d.L, D = d.D, E = d.E, V = d.V;
  const size_t ts = d.dtype == SAT_BF16 ? 2 : 4;
  BeamWS w;
  SAT_REQUIRE(beam_carve(d, R, nullptr, &w) <= workspace_bytes);
  beam_carve(d, R, (char*)workspace, &w);
  hipStream_t s = (hipStream_t)stream;
  BeamCtx c{d, *lay, params, params_lp};

  // ---- initial state for the beam_size rows (decoder.py:167-180) ----
  const int start = d.start_token;   // 0 = <start>; [CLS] under BERT (decoder.py:166-169)
  std::vector<int32_t> upl(3 * R);
  for (int i = 0; i < R; ++i) { upl[i] = i; upl[R + i] = start; float z = 0.f; memcpy(&upl[2 * R + i], &z, 4); }
  SAT_CHECK(hipMemcpyAsync(w.upl, upl.data(), 3 * R * 4, hipMemcpyHostToDevice, s));
  SAT_CHECK(hipMemcpyAsync(w.feat[0], img_features, (size_t)R * L * D * ts, hipMemcpyDeviceToDevice, s));
  SAT_CHECK((hipError_t)sat_mean_rows(w.feat[0], R, L, D, d.dtype, w.mean_f, w.mean_t, s));
  SAT_CHECK((hipError_t)lin(c, R, E, D, w.mean_t, D, c.W(lay->init_w), D, c.F(lay->init_b), w.hc0, 2 * E,
                            SAT_ACT_TANH, s, w.h_t, E, d.dtype));
  SAT_CHECK((hipError_t)lin(c, R, E, D, w.mean_t, D, c.W(lay->init_w + (long)E * D), D, c.F(lay->init_b + E),
                            w.hc0 + E, 2 * E, SAT_ACT_TANH, s, w.c, E, SAT_F32));
  if (d.attention)  // hoisted W·a + b per beam row (attention.py:16), stored in the operand dtype
    SAT_CHECK((hipError_t)lin(c, R * L, E, D, w.feat[0], D, c.W(lay->attW_w), D, c.F(lay->attW_b), w.Ws[0], E,
                              SAT_ACT_NONE, s, nullptr, 0, SAT_F32, d.dtype));

  // host-side histories (the reference's Python lists, decoder.py:171-177)
  struct Hyp { std::vector<int32_t> words; std::vector<float> alphas; };
  std::vector<Hyp> beams(R);
  for (auto& b : beams) { b.words.assign(1, start); b.alphas.assign(L, 1.0f); }
  std::vector<Hyp> done;
  std::vector<float> done_score;
  std::vector<float> tv(R), al((size_t)R * L);
  std::vector<int32_t> ti(R);
  int k = R, cur = 0, last_rows = 0;
  const long feat_row = (long)L * D * ts, ws_row = (long)L * E * ts;
  for (int step = 1;; ++step) {
    SAT_CHECK((hipError_t)beam_step(c, w, k, w.feat[cur], w.Ws[cur], w.upl + R, w.alpha, false, s));
    // step 1: every beam row is the same hypothesis -> top-k over row 0 only (decoder.py:206-207)
    hipLaunchKernelGGL(beam_topk_kernel, dim3(1), dim3(TOPK_THREADS), 0, s, (const float*)w.logits, (long)V,
                       step == 1 ? (const float*)nullptr : (const float*)(w.upl + 2 * R), step == 1 ? 1 : k, V, k,
                       w.top_val, w.top_idx);
    SAT_LAUNCH_CHECK();
    SAT_CHECK(hipMemcpyAsync(tv.data(), w.top_val, k * 4, hipMemcpyDeviceToHost, s));
    SAT_CHECK(hipMemcpyAsync(ti.data(), w.top_idx, k * 4, hipMemcpyDeviceToHost, s));
    SAT_CHECK(hipMemcpyAsync(al.data(), w.alpha, (size_t)k * L * 4, hipMemcpyDeviceToHost, s));
    SAT_CHECK(hipStreamSynchronize(s));
    last_rows = k;
    // extend, retire completed (decoder.py:210-241)
    std::vector<Hyp> next(k);
    std::vector<int> prev(k), word(k), keep;
    for (int j = 0; j < k; ++j) {
      prev[j] = ti[j] / V;
      word[j] = ti[j] - prev[j] * V;
      next[j].words = beams[prev[j]].words;
      next[j].words.push_back(word[j]);
      next[j].alphas = beams[prev[j]].alphas;
      next[j].alphas.insert(next[j].alphas.end(), al.begin() + (size_t)prev[j] * L, al.begin() + (size_t)(prev[j] + 1) * L);
      // BERT quick-fix of the reference: ids 1 / 0 end a BERT beam, 1 / 102 a vocabulary beam
      const bool end = d.bert ? (word[j] == 1 || word[j] == 0) : (word[j] == 1 || word[j] == 102);
      if (!end) keep.push_back(j);
    }
    for (int j = 0; j < k; ++j) {
      bool kept = false;
      for (int q : keep) kept |= (q == j);
      if (!kept) { done.push_back(next[j]); done_score.push_back(tv[j]); }
    }
    const int nk = (int)keep.size();
    if (nk == 0) break;
    // compact the survivors (decoder.py:243-250)
    std::vector<Hyp> nb(nk);
    for (int q = 0; q < nk; ++q) {
      nb[q] = std::move(next[keep[q]]);
      upl[q] = prev[keep[q]];
      upl[R + q] = word[keep[q]];
      memcpy(&upl[2 * R + q], &tv[keep[q]], 4);
    }
    beams.swap(nb);
    SAT_CHECK(hipMemcpyAsync(w.upl, upl.data(), 3 * R * 4, hipMemcpyHostToDevice, s));
    GatherSet g{};
    g.n = 0;
    auto add = [&](const void* src, void* dst, long rb) { g.src[g.n] = src; g.dst[g.n] = dst; g.row_bytes[g.n] = rb; ++g.n; };
    add(w.h_new, w.h_t, (long)E * ts);
    add(w.c_new, w.c, (long)E * 4);
    add(w.feat[cur], w.feat[cur ^ 1], feat_row);
    if (d.attention) add(w.Ws[cur], w.Ws[cur ^ 1], ws_row);
    SAT_CHECK((hipError_t)gather_rows(g, w.upl, nk, s));
    cur ^= 1;
    k = nk;
    if (step > max_step) break;
  }
  // the pageable H2D above may still be reading `upl` -> drain before the vector goes away
  SAT_CHECK(hipStreamSynchronize(s));
  if (done.empty()) {  // decoder.py:256-258: returns [0] and the last step's alpha rows
    out_ids[0] = 0;
    *out_len = 1;
    memcpy(out_alphas, al.data(), (size_t)last_rows * L * 4);
    *out_alpha_rows = last_rows;
    *out_score = -INFINITY;
    return 0;
  }
  size_t best = 0;   // first maximum (list.index(max(...)), decoder.py:265)
  for (size_t i = 1; i < done.size(); ++i)
    if (done_score[i] > done_score[best]) best = i;
  const Hyp& h = done[best];
  memcpy(out_ids, h.words.data(), h.words.size() * 4);
  *out_len = (int)h.words.size();
  memcpy(out_alphas, h.alphas.data(), h.alphas.size() * 4);
  *out_alpha_rows = (int)h.words.size();
  *out_score = done_score[best];
  return 0;
}

// ===== batched beam search: N images x R beams decoded together, the bookkeeping on the device ================
//
// Image n owns rows n*R .. n*R+R-1 of every per-row tensor; its first k_n rows are live.  Rows never move across
// images and the features / W·a rows never move at all (beams of an image share them): only h / c are reordered
// by parent after each step.  Instead of carrying word / alpha histories, every step stores back-pointers per
// selection slot j (the j-th of the image's top-k_n): the candidate's value, its parent row (an index into the
// rows as they were during that step) and its word; plus keep[q] = the slot that became row q of the next step.
// A completed beam is recorded as (step, slot, score) and rebuilt once at the end by walking
// slot -> parent row -> keep of the step before -> slot ... down to step 1; the alpha rows are read from the
// history the attention kernel wrote in place, [step][N*R][L].
namespace {

struct BatchWS {
  void *Ws_img, *h_img;          // per-image W·a + b [N, L, E] and h0 [N, E] (operand dtype), before the broadcast
  float *c_img;                  // c0 [N, E]
  float *hist_alpha;             // [S][NR][L]
  float *bp_val;                 // [S][NR] back-pointers per selection slot
  int32_t *bp_parent, *bp_word, *keep;
  int32_t *tok, *gidx, *bidx;    // [NR] fed words, global parent rows, broadcast map (row -> image)
  float *score;                  // [NR]
  float *part_val;               // [NR][R] per-row top-k_n of the partial stage: value, flat index in the image
  int32_t *part_idx;
  int32_t *k_n, *last_k, *done_n, *live;   // [N] live rows, live rows of the last step taken, completions; [1]
  int32_t *done_step, *done_slot;          // [N][R]
  float *done_score;
  int32_t *chain;                // [N][cap] alpha-history row of each word of the winner
  int32_t *o_ids, *o_len, *o_rows;         // device staging of the outputs
  float *o_alphas, *o_score;
};

size_t batch_carve(const SatDecoderDims& d, int N, int R, int max_step, char* base, BeamWS* w, BatchWS* b) {
  const size_t NR = (size_t)N * R, L = d.L, E = d.E, S = (size_t)max_step + 1, cap = S + 1;
  const size_t ts = d.dtype == SAT_BF16 ? 2 : 4;
  size_t off = beam_carve(d, (int)NR, base, w, 1);
  auto take = [&](auto*& p, size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    p = base ? (std::remove_reference_t<decltype(p)>)(base + off) : nullptr;
    off += bytes;
  };
  take(b->Ws_img, N * L * E * ts); take(b->h_img, N * E * ts); take(b->c_img, N * E * 4);
  take(b->hist_alpha, S * NR * L * 4);
  take(b->bp_val, S * NR * 4); take(b->bp_parent, S * NR * 4); take(b->bp_word, S * NR * 4); take(b->keep, S * NR * 4);
  take(b->tok, NR * 4); take(b->gidx, NR * 4); take(b->bidx, NR * 4); take(b->score, NR * 4);
  take(b->part_val, NR * R * 4); take(b->part_idx, NR * R * 4);
  take(b->k_n, N * 4); take(b->last_k, N * 4); take(b->done_n, N * 4); take(b->live, 4);
  take(b->done_step, NR * 4); take(b->done_slot, NR * 4); take(b->done_score, NR * 4);
  take(b->chain, N * cap * 4);
  take(b->o_ids, N * cap * 4); take(b->o_len, N * 4); take(b->o_rows, N * 4);
  take(b->o_alphas, N * cap * L * 4); take(b->o_score, N * 4);
  return off + 256;
}

__global__ void beam_batch_init_kernel(BatchWS b, int N, int R, int start) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N * R) {
    b.tok[i] = start;
    b.gidx[i] = i;
    b.bidx[i] = i / R;
    b.score[i] = 0.f;
  }
  if (i < N) { b.k_n[i] = R; b.last_k[i] = R; b.done_n[i] = 0; }
  if (i == 0) *b.live = N;
}

// ---- select / advance --------------------------------------------------------------------------------------------
// The image's top-k_n of (logits[row, v] + score[row]) over its live rows (row 0 only at step 1, where every row
// is the same hypothesis), in beam_topk_kernel's order, in two stages: one workgroup per live row takes that
// row's top-k_n (the image's top-k_n is among them: the order is total), then one workgroup per image takes the
// top-k_n of those candidates and does the bookkeeping.
__global__ void __launch_bounds__(TOPK_THREADS) beam_partial_kernel(BatchWS b, const float* __restrict__ logits, int V,
                                                                    int R, int step) {
  const int n = blockIdx.y, r = blockIdx.x, base = n * R;
  const int k = b.k_n[n];
  if (r >= (step == 1 ? (k > 0) : k)) return;   // dead row / retired image: never read
  const long at = (long)(base + r) * R;
  block_topk(logits + (long)(base + r) * V, (long)V, b.score + base + r, 1, V, k, r * V, b.part_val + at,
             b.part_idx + at);
}

// Then this step's back-pointers, the completions, and the next step's tokens / scores / parent rows.  Dead rows
// get the start token, score 0 and their own row as parent.
__global__ void __launch_bounds__(TOPK_THREADS) beam_select_kernel(BatchWS b, int V, int R, int NR, int step,
                                                                   int start, int end_a, int end_b) {
  __shared__ float sel_v[64];
  __shared__ int32_t sel_i[64];
  const int n = blockIdx.x, base = n * R;
  const int k = b.k_n[n];
  if (k == 0) return;   // retired image: its rows keep the dead-row values written when the last beam completed
  const int n_cand = (step == 1 ? 1 : k) * k;
  const float* pval = b.part_val + (long)base * R;
  const int32_t* pidx = b.part_idx + (long)base * R;
  block_topk_passes(k, [=](float pv, int pi, float& bv, int& bi) {
    for (int t = threadIdx.x; t < n_cand; t += TOPK_THREADS) {
      const int r = t / k, at = r * R + (t - r * k);
      tk_consider(pval[at], pidx[at], pv, pi, bv, bi);
    }
  }, sel_v, sel_i);
  if (threadIdx.x != 0) return;
  const long slab = (long)(step - 1) * NR + base;
  int nk = 0, nd = b.done_n[n];
  for (int j = 0; j < k; ++j) {
    const int prev = sel_i[j] / V, word = sel_i[j] - prev * V;
    b.bp_val[slab + j] = sel_v[j];
    b.bp_parent[slab + j] = prev;
    b.bp_word[slab + j] = word;
    if (word == end_a || word == end_b) {   // completed: keeps its score (decoder.py:233-241)
      b.done_step[base + nd] = step;
      b.done_slot[base + nd] = j;
      b.done_score[base + nd] = sel_v[j];
      ++nd;
    } else {                                // survivor -> row nk of the next step
      b.keep[slab + nk] = j;
      b.tok[base + nk] = word;
      b.score[base + nk] = sel_v[j];
      b.gidx[base + nk] = base + prev;
      ++nk;
    }
  }
  for (int q = nk; q < R; ++q) { b.tok[base + q] = start; b.score[base + q] = 0.f; b.gidx[base + q] = base + q; }
  b.done_n[n] = nd;
  b.last_k[n] = k;
  b.k_n[n] = nk;
  if (nk == 0) atomicSub(b.live, 1);
}

// ---- backtrack: one workgroup per image, once ------------------------------------------------------------------
// The winner is the first maximum of the done list (completion order: step, then slot).  No completion: ids = [0],
// the last step's live alpha rows, score -inf (decoder.py:256-258).
__global__ void __launch_bounds__(256) beam_backtrack_kernel(BatchWS b, int R, int NR, int L, int cap, int last_step,
                                                             int start) {
  __shared__ int rows_s, done_s;
  const int n = blockIdx.x, base = n * R;
  if (threadIdx.x == 0) {
    const int nd = b.done_n[n];
    done_s = nd > 0;
    if (nd == 0) {
      b.o_ids[(long)n * cap] = 0;
      b.o_len[n] = 1;
      b.o_rows[n] = rows_s = b.last_k[n];
      b.o_score[n] = -INFINITY;
    } else {
      int best = 0;
      for (int i = 1; i < nd; ++i)
        if (b.done_score[base + i] > b.done_score[base + best]) best = i;
      const int s = b.done_step[base + best];
      int j = b.done_slot[base + best];
      b.o_len[n] = b.o_rows[n] = rows_s = s + 1;
      b.o_score[n] = b.done_score[base + best];
      b.o_ids[(long)n * cap] = start;
      for (int t = s; t >= 1; --t) {
        const long at = (long)(t - 1) * NR + base;
        const int p = b.bp_parent[at + j];
        b.o_ids[(long)n * cap + t] = b.bp_word[at + j];
        b.chain[(long)n * cap + t] = base + p;
        if (t > 1) j = b.keep[at - NR + p];
      }
    }
  }
  __syncthreads();
  const int rows = rows_s;
  float* out = b.o_alphas + (long)n * cap * L;
  if (!done_s) {
    const float* src = b.hist_alpha + ((long)(last_step - 1) * NR + base) * L;
    for (int i = threadIdx.x; i < rows * L; i += blockDim.x) out[i] = src[i];
    return;
  }
  for (int i = threadIdx.x; i < rows * L; i += blockDim.x) {
    const int t = i / L, l = i - t * L;
    out[i] = t == 0 ? 1.0f : b.hist_alpha[((long)(t - 1) * NR + b.chain[(long)n * cap + t]) * L + l];
  }
}

int check_beam_batch(const SatDecoderDims* d, int n_images, int beam, int max_step) {
  if (check_beam(d, beam)) return SAT_ERR_INVALID;
  if (n_images < 1 || max_step < 0 || max_step > 0x7ffffff0) return SAT_ERR_INVALID;
  if ((long)n_images * beam > 1024 || beam > max_step + 2) return SAT_ERR_INVALID;
  return 0;
}

}  // namespace

extern "C" size_t sat_decoder_beam_batch_workspace_bytes(const SatDecoderDims* d, int n_images, int beam_size,
                                                         int max_step) {
  if (check_beam_batch(d, n_images, beam_size, max_step)) return 0;
  BeamWS w;
  BatchWS b;
  return batch_carve(*d, n_images, beam_size, max_step, nullptr, &w, &b);
}

extern "C" int sat_decoder_beam_search_batch(const SatDecoderDims* dp, const SatDecoderLayout* lay,
                                             const float* params, const void* params_lp, const void* img_features,
                                             int n_images, int beam_size, int max_step, void* workspace,
                                             size_t workspace_bytes, int32_t* out_ids, int* out_len,
                                             float* out_alphas, int* out_alpha_rows, float* out_score, void* stream) {
  SAT_CHECK((hipError_t)check_beam_batch(dp, n_images, beam_size, max_step));
  SAT_REQUIRE(lay && params && img_features && workspace && out_ids && out_len && out_alphas && out_alpha_rows &&
              out_score);
  SAT_REQUIRE(dp->dtype == SAT_F32 || params_lp);
  SatPolicyScope scope(dp->policy);
  SatStampScope no_stamps(nullptr, 0);
  const SatDecoderDims& d = *dp;
  const int N = n_images, R = beam_size, NR = N * R, L = d.L, D = d.D, E = d.E, V = d.V;
  const int S = max_step + 1, cap = max_step + 2;
  const size_t ts = d.dtype == SAT_BF16 ? 2 : 4;
  BeamWS w;
  BatchWS b;
  SAT_REQUIRE(batch_carve(d, N, R, max_step, nullptr, &w, &b) <= workspace_bytes);
  batch_carve(d, N, R, max_step, (char*)workspace, &w, &b);
  hipStream_t s = (hipStream_t)stream;
  BeamCtx c{d, *lay, params, params_lp};
  const int start = d.start_token;
  const int end_a = 1, end_b = d.bert ? 0 : 102;   // the reference's BERT quick-fix, as in the single-image search

  // ---- once per image: mean features, h0 / c0, W·a + b (decoder.py:167-180), then the broadcast to R rows ----
  hipLaunchKernelGGL(beam_batch_init_kernel, dim3(sat_cdiv(NR, 256)), dim3(256), 0, s, b, N, R, start);
  SAT_LAUNCH_CHECK();
  SAT_CHECK((hipError_t)sat_mean_rows(img_features, N, L, D, d.dtype, w.mean_f, w.mean_t, s));
  SAT_CHECK((hipError_t)lin(c, N, E, D, w.mean_t, D, c.W(lay->init_w), D, c.F(lay->init_b), w.hc0, 2 * E,
                            SAT_ACT_TANH, s, b.h_img, E, d.dtype));
  SAT_CHECK((hipError_t)lin(c, N, E, D, w.mean_t, D, c.W(lay->init_w + (long)E * D), D, c.F(lay->init_b + E),
                            w.hc0 + E, 2 * E, SAT_ACT_TANH, s, b.c_img, E, SAT_F32));
  GatherSet g{};
  auto add = [&](const void* src, void* dst, long rb) { g.src[g.n] = src; g.dst[g.n] = dst; g.row_bytes[g.n] = rb; ++g.n; };
  add(b.h_img, w.h_t, (long)E * ts);
  add(b.c_img, w.c, (long)E * 4);
  if (d.attention) {
    SAT_CHECK((hipError_t)lin(c, N * L, E, D, img_features, D, c.W(lay->attW_w), D, c.F(lay->attW_b), b.Ws_img, E,
                              SAT_ACT_NONE, s, nullptr, 0, SAT_F32, d.dtype));
    add(img_features, w.feat[0], (long)L * D * ts);
    add(b.Ws_img, w.Ws[0], (long)L * E * ts);
  } else {  // uniform attention: the context is the image's mean features at every step, alpha = 1 / L
    add(w.mean_t, w.ctx_t, (long)D * ts);
    SAT_CHECK((hipError_t)sat_fill_const(b.hist_alpha, (long)S * NR * L, 1.0f / (float)L, s));
  }
  SAT_CHECK((hipError_t)gather_rows(g, b.bidx, NR, s));

  // ---- the step loop: no copy and no synchronise except the early-exit poll every 8th step ----
  GatherSet r{};
  r.n = 2;
  r.src[0] = w.h_new; r.dst[0] = w.h_t; r.row_bytes[0] = (long)E * ts;
  r.src[1] = w.c_new; r.dst[1] = w.c; r.row_bytes[1] = (long)E * 4;
  int32_t live = N;
  int last_step = 0;
  for (int step = 1;; ++step) {
    SAT_CHECK((hipError_t)beam_step(c, w, NR, w.feat[0], w.Ws[0], b.tok, b.hist_alpha + (long)(step - 1) * NR * L,
                                    !d.attention, s));
    hipLaunchKernelGGL(beam_partial_kernel, dim3(step == 1 ? 1 : R, N), dim3(TOPK_THREADS), 0, s, b,
                       (const float*)w.logits, V, R, step);
    SAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_select_kernel, dim3(N), dim3(TOPK_THREADS), 0, s, b, V, R, NR, step, start, end_a, end_b);
    SAT_LAUNCH_CHECK();
    last_step = step;
    if (step > max_step) break;
    if (step % 8 == 0) {
      SAT_CHECK(hipMemcpyAsync(&live, b.live, 4, hipMemcpyDeviceToHost, s));
      SAT_CHECK(hipStreamSynchronize(s));
      if (live == 0) break;
    }
    SAT_CHECK((hipError_t)gather_rows(r, b.gidx, NR, s));
  }
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3(N), dim3(256), 0, s, b, R, NR, L, cap, last_step, start);
  SAT_LAUNCH_CHECK();
  SAT_CHECK(hipMemcpyAsync(out_ids, b.o_ids, (size_t)N * cap * 4, hipMemcpyDeviceToHost, s));
  SAT_CHECK(hipMemcpyAsync(out_len, b.o_len, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  SAT_CHECK(hipMemcpyAsync(out_alphas, b.o_alphas, (size_t)N * cap * L * 4, hipMemcpyDeviceToHost, s));
  SAT_CHECK(hipMemcpyAsync(out_alpha_rows, b.o_rows, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  SAT_CHECK(hipMemcpyAsync(out_score, b.o_score, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  SAT_CHECK(hipStreamSynchronize(s));
  return 0;
}

// Backward of the trainable top of the encoder trunk, for gfx950 (MI355X): what loss.backward() runs in the
// reference for ResNet152's last bottlenecks (encoder.py:13-17 leaves the trunk trainable; torchvision
// Bottleneck.forward) and would run for VGG19's block-5 convolutions (encoder.py:24-27) were they not frozen.
// BatchNorm stays in eval mode (train.py:122), so a unit is conv + per-channel affine + ReLU on folded weights
// (Encoder._fold) and the gradient reaches the raw parameters through the fold's chain rule.
//
//   sat_relu_mask           out = y > 0 ? g (+ add) : 0   (y null: no mask), any mix of fp32 / bf16, 16-B vectors
//   sat_conv_fold           raw conv + BN -> folded NHWC weight (compute dtype), fp32 bias, input-gradient copy
//   sat_conv_fold_backward  folded gradients -> conv.weight.grad, bn.weight.grad, bn.bias.grad (or bias.grad)
//   sat_bottleneck_backward, sat_conv3x3_relu_backward   one call per unit; C++ issues the launches
//
// Every reduction has a fixed order (sat_gemm's deterministic split-K, sat_conv3x3_wgrad, the column-sum kernels, the
// per-channel tree below): the same call gives the same bits.  No launch here is a memset or synchronises.
#include "sat_common.h"
#include "sat_internal.h"

namespace {

// ---- 8 consecutive elements of either storage dtype (i8 = index / 8) ----
__device__ __forceinline__ void ld8(const void* p, int dt, long i8, float (&v)[8]) {
  if (dt == SAT_BF16) {
    const uint4 u = ((const uint4*)p)[i8];
    const bf16* b = (const bf16*)&u;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)b[k];
  } else {
    const float4 a = ((const float4*)p)[2 * i8], b = ((const float4*)p)[2 * i8 + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}
__device__ __forceinline__ void st8(void* p, int dt, long i8, const float (&v)[8]) {
  if (dt == SAT_BF16) {
    uint4 u;
    bf16* b = (bf16*)&u;
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = (bf16)v[k];
    ((uint4*)p)[i8] = u;
  } else {
    ((float4*)p)[2 * i8] = make_float4(v[0], v[1], v[2], v[3]);
    ((float4*)p)[2 * i8 + 1] = make_float4(v[4], v[5], v[6], v[7]);
  }
}

__global__ void relu_mask_kernel(const void* __restrict__ y, int yd, const void* __restrict__ g, int gd,
                                 const void* __restrict__ add, int ad, void* __restrict__ out, int od, long n, int vec) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long n8 = vec ? n >> 3 : 0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += stride) {
    float gv[8], yv[8], av[8];
    ld8(g, gd, i, gv);
    if (add) {
      ld8(add, ad, i, av);
#pragma unroll
      for (int k = 0; k < 8; ++k) gv[k] += av[k];
    }
    if (y) {
      ld8(y, yd, i, yv);
#pragma unroll
      for (int k = 0; k < 8; ++k) gv[k] = yv[k] > 0.f ? gv[k] : 0.f;
    }
    st8(out, od, i, gv);
  }
  for (long i = (n8 << 3) + blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
    float v = ld_as_f32(g, i, gd);
    if (add) v += ld_as_f32(add, i, ad);
    if (y && !(ld_as_f32(y, i, yd) > 0.f)) v = 0.f;
    st_from_f32(out, i, od, v);
  }
}

int relu_mask_launch(const void* y, int yd, const void* g, int gd, const void* add, int ad, void* out, int od, long n,
                     hipStream_t s) {
  if (n <= 0) return 0;
  const int vec = sat_al16(y) && sat_al16(g) && sat_al16(add) && sat_al16(out);
  long blocks = ((vec ? n / 8 : n) + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, yd, g, gd, add, ad, out, od, n, vec);
  return (int)hipGetLastError();
}

// ---- the fold (Encoder._fold's arithmetic in its operation order; no contraction into FMAs) ----
// scale = gamma / sqrt(var + eps);  w' = w * scale;  b' = beta + (b - mean) * scale   (b = 0 without a conv bias)
struct FoldArgs {
  int Cout, Cin, KH, KW, dtype;
  const float* w; const float* bias;
  const float* gamma; const float* beta; const float* mean; const float* var; float eps;
  void* w_fold; float* b_fold; void* w_igrad;
};
__global__ void conv_fold_kernel(FoldArgs a) {
#pragma clang fp contract(off)   // every operation rounded on its own, as the torch sequence rounds them
  const int co = blockIdx.x, taps = a.KH * a.KW;
  const long per = (long)a.Cin * taps;
  float scale = 1.f;
  const bool bn = a.gamma != nullptr;
  if (bn) scale = a.gamma[co] / sqrtf(a.var[co] + a.eps);   // correctly rounded divide and square root
  if (threadIdx.x == 0) {
    const float b = a.bias ? a.bias[co] : 0.f;
    float bf = b;
    if (bn) {
      const float centred = b - a.mean[co];
      const float scaled = centred * scale;
      bf = a.beta[co] + scaled;
    }
    a.b_fold[co] = bf;
  }
  const float* src = a.w + co * per;   // [ci][kh][kw]
  for (long i = threadIdx.x; i < per; i += blockDim.x) {
    const int ci = (int)(i / taps), t = (int)(i - (long)ci * taps);
    const float v = bn ? src[i] * scale : src[i];
    st_from_f32(a.w_fold, (co * (long)taps + t) * a.Cin + ci, a.dtype, v);
    // the input gradient is the convolution of dZ with the taps flipped and the channels swapped
    if (a.w_igrad) st_from_f32(a.w_igrad, (ci * (long)taps + (taps - 1 - t)) * a.Cout + co, a.dtype, v);
  }
}

// ---- the fold's chain rule, one workgroup per output channel, fixed-order sums ----
//   conv.weight.grad[co,ci,kh,kw] = dW'[co,kh,kw,ci] s[co],  s = gamma rstd,  rstd = 1 / sqrt(var + eps)
//   bn.weight.grad[co] = rstd[co] (sum_k dW'[co,k] w[co,k] + db'[co] (b[co] - mean[co]))
//   bn.bias.grad[co]   = db'[co];   conv.bias.grad[co] = db'[co] s[co]
// Without BN: the layout change and bias.grad = db'.
struct FoldBwdArgs {
  int Cout, Cin, KH, KW, accumulate;
  const float* dwf; const float* dbf;
  const float* w; const float* bias; const float* gamma; const float* mean; const float* var; float eps;
  float* gw; float* gbias; float* ggamma; float* gbeta;
};
__global__ __launch_bounds__(256) void conv_fold_backward_kernel(FoldBwdArgs a) {
  const int co = blockIdx.x, taps = a.KH * a.KW, tid = threadIdx.x;
  const long per = (long)a.Cin * taps;
  const bool bn = a.gamma != nullptr;
  float rstd = 1.f, s = 1.f;
  if (bn) {
    rstd = 1.f / sqrtf(a.var[co] + a.eps);
    s = a.gamma[co] * rstd;
  }
  const float* src = a.dwf + co * per;   // [kh][kw][ci]
  const float* wr = a.w + co * per;      // [ci][kh][kw]
  float* dst = a.gw + co * per;
  float dot = 0.f;
  for (long i = tid; i < per; i += 256) {   // i over the raw layout: coalesced stores, strided reads of a small row
    const int ci = (int)(i / taps), t = (int)(i - (long)ci * taps);
    const float d = src[(long)t * a.Cin + ci];
    dot += d * wr[i];
    const float v = d * s;
    dst[i] = a.accumulate ? dst[i] + v : v;
  }
  __shared__ float red[256];
  red[tid] = dot;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {   // a fixed tree: the same sum every run
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float db = a.dbf[co];
    if (bn) {
      const float b = a.bias ? a.bias[co] : 0.f;
      const float gg = rstd * (red[0] + db * (b - a.mean[co]));
      a.ggamma[co] = a.accumulate ? a.ggamma[co] + gg : gg;
      a.gbeta[co] = a.accumulate ? a.gbeta[co] + db : db;
    }
    if (a.gbias) {
      const float gb = db * s;
      a.gbias[co] = a.accumulate ? a.gbias[co] + gb : gb;
    }
  }
}

bool train_ok(const SatConvTrain* c, bool need_igrad) {
  if (!c || !c->weight || !c->w_fold || !c->weight_grad) return false;
  if (need_igrad && !c->w_igrad) return false;
  const bool bn = c->bn_weight != nullptr;
  if (bn && (!c->bn_mean || !c->bn_var || !c->bn_weight_grad || !c->bn_bias_grad)) return false;
  if (c->bias && !c->bias_grad) return false;
  if (!bn && !c->bias) return false;   // neither BN nor a bias: no unit of the trunk
  return true;
}

int fold_backward_launch(const SatConvTrain& c, int Cout, int Cin, int KH, int KW, const float* dwf, const float* dbf,
                         int accumulate, hipStream_t s) {
  FoldBwdArgs a{};
  a.Cout = Cout; a.Cin = Cin; a.KH = KH; a.KW = KW; a.accumulate = accumulate;
  a.dwf = dwf; a.dbf = dbf;
  a.w = c.weight; a.bias = c.bias; a.gamma = c.bn_weight; a.mean = c.bn_mean; a.var = c.bn_var; a.eps = c.eps;
  a.gw = c.weight_grad; a.gbias = c.bias ? c.bias_grad : nullptr; a.ggamma = c.bn_weight_grad; a.gbeta = c.bn_bias_grad;
  hipLaunchKernelGGL(conv_fold_backward_kernel, dim3(Cout), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

inline size_t al256(size_t b) { return (b + 255) / 256 * 256; }

// carve-up of a unit backward's workspace
struct Carve {
  char* p; size_t left; bool ok = true;
  void* take(size_t bytes) {
    bytes = al256(bytes);
    if (!ok || bytes > left) { ok = false; return nullptr; }
    void* r = p; p += bytes; left -= bytes;
    return r;
  }
};

struct GemmWs { float* ws; long ws_bytes; unsigned* tickets; };
GemmWs gemm_ws(void* p) {
  GemmWs g;
  g.ws = (float*)p;
  g.ws_bytes = (long)(sat_split_gemm_ws_bytes() - kSatSplitTickets * 4);
  g.tickets = (unsigned*)((char*)p + g.ws_bytes);
  return g;
}

// C[M,N] fp32 = A(m,k) B(n,k), operands in dtype; the deterministic split-K where the split kernel takes it
int gemm_f32out(int M, int N, int K, int dtype, const void* A, long lda, int transA, const void* B, long ldb, int transB,
                float* C, const GemmWs& w, hipStream_t s) {
  SatGemm g;
  g.M = M; g.N = N; g.K = K; g.dtype = dtype;
  g.A = A; g.lda = lda; g.transA = transA;
  g.B = B; g.ldb = ldb; g.transB = transB;
  g.C = C; g.ldc = N; g.c_dtype = SAT_F32;
  g.split_ws = w.ws; g.split_ws_bytes = w.ws_bytes; g.split_tickets = w.tickets;
  return sat_gemm_launch(g, s);
}

// da [N,H,W,Cout_of_this_conv] (dtype) = conv3x3(dz, w_igrad) -- the input gradient as a forward conv on the
// flipped, channel-swapped weight (stride 1, pad 1, zero bias, no activation)
int igrad_conv(int N, int H, int W, int Cdz, int Cda, int dtype, const void* dz, const void* w_igrad,
               const float* zero_bias, void* da, hipStream_t s) {
  SatGemm g;
  g.conv = SatConvGeom{N, H, W, Cdz, 3, 3, 1, 1, H, W};
  g.M = N * H * W; g.N = Cda; g.K = 9 * Cdz; g.dtype = dtype;
  g.A = dz; g.lda = 0;
  g.B = w_igrad; g.ldb = g.K; g.transB = 0;
  g.C = da; g.ldc = Cda; g.c_dtype = dtype;
  g.bias = zero_bias;
  return sat_gemm_launch(g, s);
}

size_t es_of(int dtype) { return dtype == SAT_BF16 ? 2 : 4; }
bool dims_ok(int N, int H, int W, int Ca, int Cb, int dtype) {
  return (dtype == SAT_F32 || dtype == SAT_BF16) && N >= 1 && H >= 1 && W >= 1 && Ca >= 128 && Cb >= 128 &&
         Ca % 128 == 0 && Cb % 128 == 0 && (long)N * H * W * (Ca > Cb ? Ca : Cb) * 4 < (1L << 31);
}

}  // namespace

extern "C" int sat_relu_mask(const void* y, int y_dtype, const void* g, int g_dtype, const void* add, int add_dtype,
                             void* out, int out_dtype, int64_t n, void* stream) {
  SAT_REQUIRE(g && out && n >= 0);
  for (int d : {y_dtype, g_dtype, add_dtype, out_dtype}) SAT_REQUIRE(d == SAT_F32 || d == SAT_BF16);
  return relu_mask_launch(y, y_dtype, g, g_dtype, add, add_dtype, out, out_dtype, n, (hipStream_t)stream);
}

extern "C" int sat_conv_fold(int Cout, int Cin, int KH, int KW, int dtype, const float* weight, const float* bias,
                             const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var,
                             float eps, void* w_fold, float* b_fold, void* w_igrad, void* stream) {
  SAT_REQUIRE(Cout > 0 && Cin > 0 && KH > 0 && KW > 0 && weight && w_fold && b_fold);
  SAT_REQUIRE(dtype == SAT_F32 || dtype == SAT_BF16);
  SAT_REQUIRE(!bn_weight || (bn_bias && bn_mean && bn_var));
  FoldArgs a{};
  a.Cout = Cout; a.Cin = Cin; a.KH = KH; a.KW = KW; a.dtype = dtype;
  a.w = weight; a.bias = bias; a.gamma = bn_weight; a.beta = bn_bias; a.mean = bn_mean; a.var = bn_var; a.eps = eps;
  a.w_fold = w_fold; a.b_fold = b_fold; a.w_igrad = w_igrad;
  hipLaunchKernelGGL(conv_fold_kernel, dim3(Cout), dim3(256), 0, (hipStream_t)stream, a);
  SAT_LAUNCH_CHECK();
  return 0;
}

extern "C" int sat_conv_fold_backward(int Cout, int Cin, int KH, int KW, const float* dw_fold, const float* db_fold,
                                      const SatConvTrain* conv, int accumulate, void* stream) {
  SAT_REQUIRE(Cout > 0 && Cin > 0 && KH > 0 && KW > 0 && dw_fold && db_fold && conv);
  SAT_REQUIRE(conv->weight && conv->weight_grad);
  const bool bn = conv->bn_weight != nullptr;
  SAT_REQUIRE(!bn || (conv->bn_mean && conv->bn_var && conv->bn_weight_grad && conv->bn_bias_grad));
  SAT_REQUIRE(!conv->bias || conv->bias_grad);
  return fold_backward_launch(*conv, Cout, Cin, KH, KW, dw_fold, db_fold, accumulate != 0, (hipStream_t)stream);
}

// ---- workspaces -------------------------------------------------------------------------------------------
static size_t unit_common_bytes(long P, int Cmax, long dw_elems) {
  return al256((size_t)dw_elems * 4) + al256((size_t)Cmax * 4) * 2 +          // dW', db', zero bias
         al256(sat_colsum_scratch_floats((int)P, Cmax) * 4) + al256(sat_split_gemm_ws_bytes());
}

extern "C" size_t sat_bottleneck_backward_workspace_bytes(int N, int H, int W, int Cin, int Cmid, int dtype,
                                                          const SatPolicy* policy) {
  if (!dims_ok(N, H, W, Cin, Cmid, dtype)) return 0;
  const long P = (long)N * H * W;
  const size_t es = es_of(dtype);
  const int Cmax = Cin > Cmid ? Cin : Cmid;
  const long dw = (long)Cin * Cmid > 9L * Cmid * Cmid ? (long)Cin * Cmid : 9L * Cmid * Cmid;
  const size_t wg = sat_conv3x3_wgrad_workspace_bytes(N, H, W, Cmid, Cmid, dtype, policy);
  if (!wg) return 0;
  return al256(P * Cin * es) + 3 * al256(P * Cmid * es) + al256(P * Cmax * 4) + unit_common_bytes(P, Cmax, dw) +
         al256(wg);
}

extern "C" size_t sat_conv3x3_relu_backward_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype,
                                                            const SatPolicy* policy) {
  if (!dims_ok(N, H, W, Cin, Cout, dtype)) return 0;
  const long P = (long)N * H * W;
  const int Cmax = Cin > Cout ? Cin : Cout;
  const size_t wg = sat_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout, dtype, policy);
  if (!wg) return 0;
  return al256(P * Cout * es_of(dtype)) + unit_common_bytes(P, Cmax, 9L * Cin * Cout) + al256(wg);
}

// ---- unit backwards ---------------------------------------------------------------------------------------
/* see include/sat_hip.h */
extern "C" int sat_bottleneck_backward(int N, int H, int W, int Cin, int Cmid, int dtype, const void* x, const void* a1,
                                       const void* a2, const void* y, const SatConvTrain* c1, const SatConvTrain* c2,
                                       const SatConvTrain* c3, const void* dy, void* dx, int accumulate,
                                       void* workspace, size_t workspace_bytes, const SatPolicy* policy,
                                       void* stream) {
  SAT_REQUIRE(x && a1 && a2 && y && dy && workspace && dims_ok(N, H, W, Cin, Cmid, dtype));
  SAT_REQUIRE(train_ok(c1, false) && train_ok(c2, true) && train_ok(c3, false));
  SAT_REQUIRE(sat_al16(x) && sat_al16(a1) && sat_al16(a2) && sat_al16(y) && sat_al16(dy) && sat_al16(dx) &&
              ((uintptr_t)workspace & 255) == 0);
  SAT_REQUIRE(workspace_bytes >= sat_bottleneck_backward_workspace_bytes(N, H, W, Cin, Cmid, dtype, policy));
  SatPolicyScope scope(policy);
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)N * H * W;
  const size_t es = es_of(dtype);
  const int Cmax = Cin > Cmid ? Cin : Cmid;
  const long dw_elems = (long)Cin * Cmid > 9L * Cmid * Cmid ? (long)Cin * Cmid : 9L * Cmid * Cmid;
  const size_t wg_bytes = sat_conv3x3_wgrad_workspace_bytes(N, H, W, Cmid, Cmid, dtype, policy);
  Carve cv{(char*)workspace, workspace_bytes};
  void* dz3 = cv.take(P * Cin * es);
  void* dz2 = cv.take(P * Cmid * es);
  void* dz1 = cv.take(P * Cmid * es);
  void* da1 = cv.take(P * Cmid * es);
  float* G = (float*)cv.take(P * Cmax * 4);
  float* dwf = (float*)cv.take((size_t)dw_elems * 4);
  float* dbf = (float*)cv.take((size_t)Cmax * 4);
  float* zb = (float*)cv.take((size_t)Cmax * 4);
  float* cs = (float*)cv.take(sat_colsum_scratch_floats((int)P, Cmax) * 4);
  void* gws = cv.take(sat_split_gemm_ws_bytes());
  void* wgws = cv.take(wg_bytes);
  SAT_REQUIRE(cv.ok);
  const GemmWs gw = gemm_ws(gws);
  const int acc = accumulate != 0;

  // c3 + residual + ReLU: dZ3 = [y > 0] dY;  dW3' = dZ3^T a2;  db3' = column sums of dZ3
  SAT_CHECK((hipError_t)relu_mask_launch(y, dtype, dy, dtype, nullptr, dtype, dz3, dtype, P * Cin, s));
  SAT_CHECK((hipError_t)gemm_f32out(Cin, Cmid, (int)P, dtype, dz3, Cin, 1, a2, Cmid, 1, dwf, gw, s));
  SAT_CHECK((hipError_t)sat_colsum(dz3, dtype, Cin, (int)P, Cin, dbf, 0, nullptr, cs, s));
  SAT_CHECK((hipError_t)fold_backward_launch(*c3, Cin, Cmid, 1, 1, dwf, dbf, acc, s));
  // dA2 = dZ3 W3';  c2 + ReLU: dZ2 = [a2 > 0] dA2, rounded once to the compute dtype
  SAT_CHECK((hipError_t)gemm_f32out((int)P, Cmid, Cin, dtype, dz3, Cin, 0, c3->w_fold, Cmid, 1, G, gw, s));
  SAT_CHECK((hipError_t)relu_mask_launch(a2, dtype, G, SAT_F32, nullptr, dtype, dz2, dtype, P * Cmid, s));
  // dW2' (the 3x3 weight gradient), db2'
  {
    const int e = sat_conv3x3_wgrad(N, H, W, Cmid, Cmid, dtype, a1, dz2, dwf, 0, wgws, wg_bytes, policy, stream);
    if (e) return e;
  }
  SAT_CHECK((hipError_t)sat_colsum(dz2, dtype, Cmid, (int)P, Cmid, dbf, 0, nullptr, cs, s));
  SAT_CHECK((hipError_t)fold_backward_launch(*c2, Cmid, Cmid, 3, 3, dwf, dbf, acc, s));
  // dA1 = conv3x3(dZ2, flipped W2');  c1 + ReLU: dZ1 = [a1 > 0] dA1
  SAT_CHECK((hipError_t)sat_zero_rows(zb, Cmax, 1, Cmax, s));
  SAT_CHECK((hipError_t)igrad_conv(N, H, W, Cmid, Cmid, dtype, dz2, c2->w_igrad, zb, da1, s));
  SAT_CHECK((hipError_t)relu_mask_launch(a1, dtype, da1, dtype, nullptr, dtype, dz1, dtype, P * Cmid, s));
  // dW1' = dZ1^T x, db1'
  SAT_CHECK((hipError_t)gemm_f32out(Cmid, Cin, (int)P, dtype, dz1, Cmid, 1, x, Cin, 1, dwf, gw, s));
  SAT_CHECK((hipError_t)sat_colsum(dz1, dtype, Cmid, (int)P, Cmid, dbf, 0, nullptr, cs, s));
  SAT_CHECK((hipError_t)fold_backward_launch(*c1, Cmid, Cin, 1, 1, dwf, dbf, acc, s));
  // the block's input gradient: dX = dZ1 W1' + dZ3 (the identity shortcut), rounded once
  if (dx) {
    SAT_CHECK((hipError_t)gemm_f32out((int)P, Cin, Cmid, dtype, dz1, Cmid, 0, c1->w_fold, Cin, 1, G, gw, s));
    SAT_CHECK((hipError_t)relu_mask_launch(nullptr, dtype, G, SAT_F32, dz3, dtype, dx, dtype, P * Cin, s));
  }
  return 0;
}

/* see include/sat_hip.h */
extern "C" int sat_conv3x3_relu_backward(int N, int H, int W, int Cin, int Cout, int dtype, const void* x,
                                         const void* y, const SatConvTrain* c, const void* dy, void* dx,
                                         int accumulate, void* workspace, size_t workspace_bytes,
                                         const SatPolicy* policy, void* stream) {
  SAT_REQUIRE(x && y && dy && workspace && dims_ok(N, H, W, Cin, Cout, dtype) && train_ok(c, dx != nullptr));
  SAT_REQUIRE(sat_al16(x) && sat_al16(y) && sat_al16(dy) && sat_al16(dx) && ((uintptr_t)workspace & 255) == 0);
  SAT_REQUIRE(workspace_bytes >= sat_conv3x3_relu_backward_workspace_bytes(N, H, W, Cin, Cout, dtype, policy));
  SatPolicyScope scope(policy);
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)N * H * W;
  const int Cmax = Cin > Cout ? Cin : Cout;
  const size_t wg_bytes = sat_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout, dtype, policy);
  Carve cv{(char*)workspace, workspace_bytes};
  void* dz = cv.take(P * Cout * es_of(dtype));
  float* dwf = (float*)cv.take((size_t)9 * Cin * Cout * 4);
  float* dbf = (float*)cv.take((size_t)Cmax * 4);
  float* zb = (float*)cv.take((size_t)Cmax * 4);
  float* cs = (float*)cv.take(sat_colsum_scratch_floats((int)P, Cmax) * 4);
  cv.take(sat_split_gemm_ws_bytes());   // (the layout shared with the bottleneck's; no 1x1 product here)
  void* wgws = cv.take(wg_bytes);
  SAT_REQUIRE(cv.ok);
  // conv + bias + ReLU: dZ = [y > 0] dY;  dW' (the 3x3 weight gradient);  db' = column sums;  dX = conv3x3(dZ, flipped W')
  SAT_CHECK((hipError_t)relu_mask_launch(y, dtype, dy, dtype, nullptr, dtype, dz, dtype, P * Cout, s));
  {
    const int e = sat_conv3x3_wgrad(N, H, W, Cin, Cout, dtype, x, dz, dwf, 0, wgws, wg_bytes, policy, stream);
    if (e) return e;
  }
  SAT_CHECK((hipError_t)sat_colsum(dz, dtype, Cout, (int)P, Cout, dbf, 0, nullptr, cs, s));
  SAT_CHECK((hipError_t)fold_backward_launch(*c, Cout, Cin, 3, 3, dwf, dbf, accumulate != 0, s));
  if (dx) {
    SAT_CHECK((hipError_t)sat_zero_rows(zb, Cmax, 1, Cmax, s));
    SAT_CHECK((hipError_t)igrad_conv(N, H, W, Cout, Cin, dtype, dz, c->w_igrad, zb, dx, s));
  }
  return 0;
}

/*
 * sat_hip.h — C ABI of the MI355X-native Show-Attend-and-Tell training path.
 *
 * The reference (yvokeller/Show-Attend-and-Tell) has no FFI: its hot path is the
 * PyTorch nn.Module API (encoder.py, attention.py, decoder.py) called from the
 * inner loop of train.py.  This header is the boundary *below* that API: every
 * entry point replaces a PyTorch op sequence of the reference, cited as
 * file:line.  The Python package (show-attend-and-tell_amd/, imported as
 * ``sat_amd``) keeps the reference module API and binds these symbols with
 * ctypes; a maintainer-side binding is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All tensor arguments are DEVICE pointers allocated by the caller (PyTorch's
 *     caching allocator owns every buffer, including workspaces).
 *   - ``stream`` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream);
 *     every call is asynchronous on it and performs no host synchronisation, so
 *     calls are legal inside hipGraph stream capture.
 *   - Return value: 0 on success, SAT_ERR_INVALID for a rejected shape/argument,
 *     otherwise the hipError_t of the failing HIP call.  The Python layer raises
 *     RuntimeError on non-zero, as the reference raises Python exceptions.
 *   - dtype: SAT_F32 = exact fp32 path (parity mode, fp32-input MFMA);
 *            SAT_BF16 = bf16 operands, fp32 accumulation (performance mode).
 *   - Layouts are row-major; image tensors are NHWC (channels last), which makes
 *     the encoder's permute(0,2,3,1).view(B,-1,C) (encoder.py:37-39) free.
 */
#ifndef SAT_HIP_H_
#define SAT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAT_ABI_VERSION 9

enum { SAT_F32 = 0, SAT_BF16 = 1 };
enum { SAT_ACT_NONE = 0, SAT_ACT_RELU = 1, SAT_ACT_TANH = 2, SAT_ACT_SIGMOID = 3 };
enum { SAT_OK = 0, SAT_ERR_INVALID = 9001 };

/* Implicit-GEMM convolution geometry (NHWC input, [Cout][KH][KW][C] weights). */
typedef struct {
  int N, H, W, C, KH, KW, stride, pad, OH, OW;
} SatConvGeom;

/* Per-call kernel selection.  Every field 0 = the library's choice (what the product runs); the
 * other values force or exclude one kernel for a single call -- the tests that compare two kernels bit
 * for bit, and A/B measurements.  Passed by pointer (nullable = all defaults) to every entry point that
 * dispatches among kernels: SatGemmArgs.policy, sat_conv2d_nhwc, SatDecoderDims.policy.  There is no
 * process-global tuning state: two callers in one process never see each other's policy. */
typedef struct {
  int conv_pipe;        /* pipelined 256x128 conv / GEMM kernel: 0 auto (long-K, chip-filling problems), 1 off,
                         * 2 every eligible problem */
  int conv_stream;      /* weight-stationary 1x1 kernel (K <= 512): 0 auto, 1 off, 2 every eligible */
  int conv3x3_ws;       /* 64 -> 64 3x3 weight-stationary halo kernel: 0 on, 1 off */
  int conv_slices;      /* layer3 c1 / c2 half-image kernels (sat_conv1x1_frag, sat_conv3x3_frag at 14x14): 0 auto
                         * (two 128-channel slices per half image when B < 64), 1 one workgroup per half image, 2 the
                         * slices; sat_conv3x3_frag at 7x7: 0 auto (two images per workgroup when B > 64), 1 two
                         * images, 2 one image per workgroup */
  int skinny;           /* register-direct skinny GEMM (M <= 128): 0 the decoder's split products, 1 off,
                         * 2 every eligible problem */
  int gemm_stages;      /* LDS ring depth of the bf16 tile kernel: 0 auto, 2, 3 */
  int gemm_tile;        /* tile kernel configuration: 0 auto, 1 = 128x128 / 8 waves, 2 = 128x64 / 8, 3 = 128x128 / 4,
                         * 4 = 128x256 / 8, 5 = 256x128 / 8 (k-major operands use 1 or 3) */
  int gemm_linear_order;/* 1 = plain tile order instead of the XCD-aware one (tile kernel) */
  int gemm_epilogue;    /* bf16-output epilogue of 128-row tiles: 0 bf16 LDS epilogue for every eligible launch,
                         * 1 for residual launches only, 2 fp32 tile staged in LDS */
  int split_gemm;       /* bf16 products with fp32 output and a k-major operand (the decoder's batched weight / input
                         * gradients; gemmsplit.hip: deterministic split-K, no atomics): 0 auto, 1 off (the tile
                         * kernel), 2 128-row tiles only, 3 256-row tiles only; 4 as 0 with every product launched on
                         * its own (no grouped launches: the A/B of sat_gemm_group and the decoder backward's groups) */
  int split_k;          /* split_gemm: 0 the planner's split count, n > 0 exactly n splits when the shape allows */
  int attn_bwd;         /* attention backward per decoder step: 0 auto, 1 the two-launch form */
  int attn_bwd_chunks;  /* split attention backward: slot chunks per batch row (0 auto: ~256 workgroups) */
  int attn_pipe;        /* attention forward / split backward over more slots than one batch of loads (L = 196):
                         * 0 auto (slot batches double-buffered), 1 one batch at a time */
  int decoder_splits[4];/* split-K counts of the per-step bf16 decoder GEMMs -- h: [U; f_beta; W_hh] h, c: context
                         * part of the gate GEMM, g: dL/d(gated context), dh: recurrent dL/dh; 0 = automatic; a count
                         * that does not divide K into whole 64-deep k-tiles, or 1 on a K >= 1024 product (it would
                         * take the tile kernel's fp32-atomic split-K), keeps the automatic count */
  int greedy_step;      /* bf16 forward without teacher forcing (decoder.py:118-133 per step): 0 the fused greedy step
                         * (token table for the embedding half of the gate GEMM, dropout in the LSTM kernel, f_z beside
                         * the context GEMM, f_h + combine in one launch, the vocabulary head with in-launch argmax
                         * partials), 1 the per-op form (a GEMM / elementwise launch per reference op) */
  int embed_grad;       /* dense embedding gradient (decoder.py:87,133 nn.Embedding backward): 0 per-token sums in row
                         * order (sorted segments: bit-reproducible), 1 fp32 atomics */
  /* diagnostics (bench.py's in-step kernel timing): a device buffer; when non-null and stamps[0] != 0 (the
   * enable word, read by the kernels at every launch -- so a captured hipGraph can be replayed with stamps
   * on or off), every workgroup w < stamp_capacity of the call's launch writes {first-wave start, last-wave
   * end} of the device's 100 MHz real-time counter to stamps[2 + 2 w], stamps[3 + 2 w]; the launch's span
   * = max(end) - min(start).  The decoder calls lay out kStampGroups x (T-1) such slots of
   * 2 (stamp_capacity + 1) words, one per per-step kernel group and step (decoder.hip). */
  uint64_t* stamps;
  int stamp_capacity;
} SatPolicy;

/* Generic GEMM:  C[m,n] = act(alpha*sum_k A(m,k)B(n,k) + bias[n] + add1[m,n] + beta*C[m,n]),
 * A(m,k) = transA ? A[k*lda+m] : A[m*lda+k];  B(n,k) = transB ? B[k*ldb+n] : B[n*ldb+k].
 * Optional aux output receives the same (post-activation) value in aux_dtype.
 * Replaces torch.nn.Linear forward/backward (e.g. attention.py:15-16,
 * decoder.py:99,125,143-146,151-158).
 * workspace (nullable, device, workspace_bytes >= sat_gemm_workspace_bytes()): lets a product with fp32 output and
 * a k-major operand split K over workgroups with a deterministic in-launch reduction (partial tiles + arrival
 * tickets, zeroed by the call itself); without it such a product runs unsplit.  One workspace serves calls that
 * are ordered on one stream. */
typedef struct {
  int M, N, K, dtype;
  const void* A; int64_t lda; int transA;
  const void* B; int64_t ldb; int transB;
  void* C; int64_t ldc; int c_dtype;
  float alpha, beta;
  const float* bias;
  const void* add1; int64_t ld_add1; int add1_dtype;
  int act;
  void* aux; int64_t ld_aux; int aux_dtype;
  const SatPolicy* policy;    /* nullable: library defaults */
  void* workspace; int64_t workspace_bytes;
} SatGemmArgs;

/* Decoder problem description (decoder.py:9-67 constructor flags + shapes). */
typedef struct {
  int B, L, D, E, V, T;       /* T = caption length; the decoder runs T-1 steps (decoder.py:77) */
  int tf, ado, attention, bert, training;
  int dtype;
  int start_token;            /* 0 = <start> (decoder.py:82); 101 = [CLS] (decoder.py:80) */
  int has_dropout_mask;       /* training: 1 = use the caller's keep-mask, 0 = draw from seed */
  uint64_t seed;
  /* optional device counter: when set, masks are drawn from (seed ^ *seed_ptr) and the forward
   * increments *seed_ptr on the stream, so a hipGraph replay draws fresh masks every step. */
  uint64_t* seed_ptr;
  /* workgroups the per-step split-K GEMMs aim for (0 = the library default, 192): per call, so two
   * decoders in one process can differ and a captured graph keeps the value its workspace was sized with */
  int split_target;
  const SatPolicy* policy;    /* nullable: library defaults (must be the same for a forward and its backward) */
} SatDecoderDims;

/* Element offsets of every decoder parameter inside one flat fp32 buffer.  Keys
 * map to the reference state_dict.  Groups the kernels read as
 * one matrix are adjacent:
 *   init_w = [init_h.weight ; init_c.weight] [2E,D],  init_b = [init_h.bias ; init_c.bias]
 *   hcat_w = [attention.U.weight ; f_beta.weight ; lstm.weight_hh] [E+D+4E, E]
 *   hcat_b = [attention.U.bias ; f_beta.bias ; lstm.bias_hh]. */
typedef struct {
  int64_t embedding, init_w, init_b, hcat_w, hcat_b, attW_w, attW_b, v_w, v_b, wih, bih;
  int64_t fh_w, fh_b, fz_w, fz_b, fout_w, fout_b, do_w, do_b;
  int64_t total;
  /* bf16 mode, optional (-1 = absent): element offsets in params_lp of transposed copies
   *   wih_ctx_t = W_ih[:, E:]^T [D, 4E] and hcat_t = hcat_w^T [E, E+D+4E]
   * (sat_decoder_refresh_transposed writes them from the shadow's own rows after every weight update); the
   * BPTT's dL/d(gated context) and dL/dh products then read k-contiguous weights (the skinny kernel) */
  int64_t wih_ctx_t, hcat_t;
} SatDecoderLayout;

int sat_abi_version(void);
const char* sat_error_string(int code);

/* --- generic building blocks -------------------------------------------- */
int sat_gemm(const SatGemmArgs* args, void* stream);
size_t sat_gemm_workspace_bytes(void);

/* Independent products as one launch (the decoder backward's batched weight / input gradients; gemmsplit.hip).
 * sat_gemm_group runs args[0 .. n) (n <= 8), each under its own args[i].policy: the products sat_gemm would run on
 * the deterministic split-K kernel share one grid, planned jointly (tile height and split count per product;
 * policy->split_gemm = 2 / 3 and policy->split_k force them as for sat_gemm, and a product in a group computes the
 * same bits as sat_gemm with the same tile height and split count); the others run as sat_gemm would run them,
 * after the group.  No product may read another's output.  workspace (device, >= sat_gemm_group_workspace_bytes();
 * args[i].workspace is ignored): partial tiles and arrival tickets, the tickets zeroed by the call.
 *
 * sat_gemm_group_plan is the planner alone (host code, no device): shapes[i] with tile_rows (0, 128, 256) and splits
 * (0 = the planner's) forced or free, the partial-tile bytes and the tickets the set may use.  plan[i] receives the
 * product's tile height, split count, K range per split (kchunk), tile grid, its blocks [first_block, first_block
 * + blocks) in the launch, and for splits > 1 its own slab region (bytes) and ticket range.  fallback = 1: the
 * product is not in the launch (a forced split count the shape or the remaining workspace cannot hold) and runs on
 * its own.  sat_gemm_group_block maps a block of the launch back to its work item (-1 product: none).
 * sat_gemm_group_launches: grouped launches this process has issued so far, sat_gemm_group's and the decoder
 * backward's (one captured into a graph counts once, at capture). */
typedef struct {
  int M, N, K;
  int tile_rows, splits;
} SatGemmGroupShape;
typedef struct {
  int tile_rows, splits, kchunk, tiles_m, tiles_n;
  int first_block, blocks;
  int64_t slab_offset, slab_bytes;
  int ticket_offset, tickets;
  int fallback;
} SatGemmGroupPlan;
int sat_gemm_group(const SatGemmArgs* args, int n, void* workspace, int64_t workspace_bytes, void* stream);
size_t sat_gemm_group_workspace_bytes(void);
int sat_gemm_group_plan(const SatGemmGroupShape* shapes, int n, int64_t slab_bytes, int tickets, SatGemmGroupPlan* plan);
int sat_gemm_group_block(const SatGemmGroupPlan* plan, int n, int block, int* product, int* tile_m, int* tile_n,
                         int* split);
int64_t sat_gemm_group_launches(void);
/* elementwise cast between SAT_F32 and SAT_BF16 storage (n elements). */
int sat_cast(const void* x, int x_dtype, void* y, int y_dtype, int64_t n, void* stream);

/* mean over L: a [B,L,D] -> out_f32 [B,D] (nullable) and out_t [B,D] in dtype (nullable);
 * img_features.mean(dim=1) of decoder.py:139 / the uniform-attention context of decoder.py:104. */
int sat_mean_rows_abi(const void* a, int B, int L, int D, int dtype, float* out_f32, void* out_t, void* stream);

/* --- encoder (encoder.py:33-40 with the torchvision trunks) ------------- */
/* NCHW fp32 image batch -> NHWC (dtype) with channels zero-padded to Cp. */
int sat_nchw_to_nhwc(int N, int C, int H, int W, int Cp, int dtype, const float* x, void* y, void* stream);
/* NCHW fp32 (C <= 4, H and W even) -> space-to-depth NHWC [N, H/2, W/2, 16] (dtype): channel
 * (sy*2 + sx)*C + c holds x[n, c, 2*by + sy, 2*bx + sx], channels 4C..15 zero.  Feeds the ResNet152
 * stem as a 4x4 / stride-1 / top-left-pad-2 conv (encoder.py:13-17 conv1, re-laid out). */
int sat_nchw_to_s2d(int N, int C, int H, int W, int dtype, const float* x, void* y, void* stream);
/* y = act(conv(x, w) + bias [+ residual]); x NHWC [N,H,W,C], y NHWC [N,OH,OW,Cout]; pad is the
 * top/left padding, OH/OW are taken as given (bottom/right padding = whatever they imply);
 * covers Conv2d+ReLU (VGG19) and Conv2d+BatchNorm(eval, folded)+[residual]+ReLU (ResNet152). */
int sat_conv2d_nhwc(const SatConvGeom* g, int Cout, int dtype, const void* x, const void* w,
                    const float* bias, const void* residual, int relu, void* y, const SatPolicy* policy,
                    void* stream);
/* Weight re-layout for register-direct MFMA fragment loads (once per weight version):
 * src [N][K] bf16 row-major -> dst [N/16][K/32][64][8], lane l = 16*(k8 % 4) + (n % 16) of block
 * (n / 16, k / 32) holding src[n][32*(k/32) + 8*(l >> 4) .. +8].  N % 16 == 0, K % 32 == 0. */
int sat_mfma_frag_layout(int N, int K, const void* src, void* dst, void* stream);
/* 1 if sat_bottleneck_fused runs this geometry (today: bf16, 14x14, Cin 1024, Cmid 256 -- the 35
 * identity blocks of ResNet152 layer3), else 0. */
int sat_bottleneck_fused_supported(int H, int W, int Cin, int Cmid, int dtype);
/* One torchvision Bottleneck with identity residual and stride 1, eval-BN folded (encoder.py:13-17,
 * 33-36 through torchvision): y = relu(c3(relu(c2(relu(c1(x))))) + x) in ONE launch; c1/c2 outputs
 * stay on chip.  x, y NHWC [N,H,W,Cin] (x != y); w1f/w2f/w3f: sat_mfma_frag_layout of the folded
 * [Cmid][Cin], [Cmid][3*3*Cmid] (tap-major) and [Cin][Cmid] weights; b1/b2/b3 folded fp32 biases.
 * Bit-identical to the three sat_conv2d_nhwc launches it replaces. */
int sat_bottleneck_fused(int N, int H, int W, int Cin, int Cmid, int dtype, const void* x, const void* w1f,
                         const float* b1, const void* w2f, const float* b2, const void* w3f, const float* b3,
                         void* y, const SatPolicy* policy, void* stream);
/* 1 if sat_conv3x3_frag runs this geometry (bf16: 14x14 C 256, 28x28 C 128, 7x7 C 512 -- the c2 of ResNet152's
 * layer3 / layer2 / layer4 identity blocks -- and VGG19's 14x14 C 512 block-5 and 112x112 C 128 block-2 convs), else 0. */
int sat_conv3x3_frag_supported(int H, int W, int C, int dtype);
/* 3x3 / stride 1 / pad 1 conv C -> C + folded bias + ReLU (a bottleneck's c2, encoder.py:13-17 through
 * torchvision), one workgroup per half image (14x14), 7-row band (28x28) or one / two whole images x a
 * 128-channel slice (7x7) with its input rows staged once in LDS and the weights streamed register-direct.  x, y NHWC [N,H,W,C] (x != y); wf: sat_mfma_frag_layout of the folded
 * [C][3*3*C] (tap-major) weight; b: fp32 bias.  Bit-identical to sat_conv2d_nhwc on the same operands. */
int sat_conv3x3_frag(int N, int H, int W, int C, int dtype, const void* x, const void* wf, const float* b, void* y,
                     const SatPolicy* policy, void* stream);
/* 1 if sat_conv1x1_frag runs this geometry (today: bf16, 14x14, Cin 1024, Cout 256 -- the c1 of ResNet152's
 * layer3 identity blocks), else 0. */
int sat_conv1x1_frag_supported(int H, int W, int Cin, int Cout, int dtype);
/* 1x1 conv Cin -> Cout + folded bias + ReLU (a bottleneck's c1, encoder.py:13-17 through torchvision), one
 * workgroup per half image: input slabs by LDS-DMA, weights register-direct.  x NHWC [N,H,W,Cin], y
 * [N,H,W,Cout] (x != y); wf: sat_mfma_frag_layout of the folded [Cout][Cin] weight.  Bit-identical to
 * sat_conv2d_nhwc. */
int sat_conv1x1_frag(int N, int H, int W, int Cin, int Cout, int dtype, const void* x, const void* wf,
                     const float* b, void* y, const SatPolicy* policy, void* stream);
/* A bottleneck's c3 and the next bottleneck's c1 in ONE launch (encoder.py:13-17, 33-36 through torchvision; the
 * ResNet152 layer1 / layer2 blocks): y [M,N] = relu(x [M,K] . w [N,K]^T + bias + residual [M,N]) and
 * x1 [M,N2] = relu(y . w1 [N2,N]^T + b1), M = the NHWC pixels of a 1x1 / stride-1 conv.  The c1 is computed from
 * y's finished tile while it is still on chip (csrc/convstream.hip), so y is not read back.  Both outputs are
 * bit-identical to the two sat_conv2d_nhwc launches.
 * _supported: 1 if the chained kernel takes the shape -- bf16, (K, N, N2) one of (64, 256, 64), (64, 256, 128),
 * (128, 512, 128), M * N < 2^31 -- under the policy's conv_stream: 0 auto (HBM-bound problems: at least two 32 / 64-row
 * items per CU), 1 never, 2 every such shape.
 * sat_conv1x1_chain runs the chained kernel when _supported, residual is non-null and every pointer is 16-byte
 * aligned; otherwise it issues the two launches itself (so it succeeds wherever they would). */
int sat_conv1x1_chain_supported(int64_t M, int K, int N, int N2, int dtype, const SatPolicy* policy);
int sat_conv1x1_chain(int64_t M, int K, int N, int N2, int dtype, const void* x, const void* w, const float* bias,
                      const void* residual, void* y, const void* w1, const float* b1, void* x1,
                      const SatPolicy* policy, void* stream);
/* The c3 of a stage's first bottleneck with its projection shortcut computed inside the launch (ResNet152 layer1 /
 * layer2 block 0): y [M,N] = relu(x [M,K] . w [N,K]^T + bias + bf16(xin_m . wp [N,Kp]^T + bp)), where xin
 * NHWC [n,H,W,Kp] is the block's input and row m = (img, oh, ow) reads its pixel (img, oh * stride, ow * stride),
 * OH = (H - 1) / stride + 1, M = n * OH * OW.  The downsample conv's output is formed in registers from xin's tile
 * (csrc/convstream.hip) and never written.  With N2 > 0 the launch also computes the next bottleneck's c1 as
 * sat_conv1x1_chain does: x1 [M,N2] = relu(y . w1 [N2,N]^T + b1); N2 = 0: w1, b1, x1 are ignored.  Bit-identical to
 * the sat_conv2d_nhwc launches (downsample, then c3 with residual, then c1).
 * _supported: 1 if a projection kernel takes the shape -- bf16, (K, N, Kp, stride, N2) one of (64, 256, 64, 1, 0),
 * (64, 256, 64, 1, 64), (128, 512, 256, 2, 0), M * N < 2^31 -- under the policy's conv_stream as for sat_conv2d_nhwc's
 * stream kernel (N2 = 0) or sat_conv1x1_chain (N2 > 0).
 * sat_conv1x1_proj has no second path: it fails with an invalid-argument code unless _supported, xin is under
 * 2 GiB and every pointer is 16-byte aligned; the caller then issues the downsample launch itself. */
int sat_conv1x1_proj_supported(int64_t M, int K, int N, int Kp, int stride, int N2, int dtype, const SatPolicy* policy);
int sat_conv1x1_proj(int n, int H, int W, int stride, int K, int N, int Kp, int N2, int dtype, const void* x,
                     const void* w, const float* bias, const void* xin, const void* wp, const float* bp, void* y,
                     const void* w1, const float* b1, void* x1, const SatPolicy* policy, void* stream);
/* ResNet152's stem as ONE launch: the conv (+ folded BatchNorm + ReLU) and the MaxPool2d that follows it
 * (encoder.py:13-17 through torchvision: conv1, bn1, relu, maxpool).  g, Cout, x, w, bias, relu as for
 * sat_conv2d_nhwc; y NHWC [N, OH / 2, OW / 2, Cout] is the pooled tensor -- the conv's own output is never written.
 * Bit-identical to sat_conv2d_nhwc followed by sat_maxpool2d_nhwc.
 * _supported: 1 for bf16, relu, the 4x4 / stride 1 / pad 2 stem over the 16-channel space-to-depth input at width 112
 * (OH = H even, OW = W), Cout 64, pool (3, 2, 1), input and conv output under 2 GiB, and a policy that leaves the
 * weight-stationary conv kernel on (conv3x3_ws != 1).
 * sat_conv_stem_pool has no second path: it fails with an invalid-argument code unless _supported and every pointer
 * is 16-byte aligned; the caller then issues the conv and the pool itself. */
int sat_conv_stem_pool_supported(const SatConvGeom* g, int Cout, int dtype, int relu, int pool_k, int pool_stride,
                                 int pool_pad, const SatPolicy* policy);
int sat_conv_stem_pool(const SatConvGeom* g, int Cout, int dtype, const void* x, const void* w, const float* bias,
                       int relu, int pool_k, int pool_stride, int pool_pad, void* y, const SatPolicy* policy,
                       void* stream);
/* MaxPool2d (floor mode, -inf padding) on NHWC. */
int sat_maxpool2d_nhwc(int N, int H, int W, int C, int k, int stride, int pad, int dtype,
                       const void* x, void* y, int OH, int OW, void* stream);

/* --- encoder backward (the trainable top of the trunk) ------------------- */
/* Weight gradient of a 3x3 / stride-1 / pad-1 convolution (autograd's conv.weight gradient for the c2 of a
 * torchvision Bottleneck, Bottleneck.forward through encoder.py:13-17, and for VGG19's block-5 convolutions,
 * encoder.py:24-27):
 *   dw[co][kh][kw][ci] (+)= sum over (n, oh, ow) of dz[n, oh, ow, co] * x[n, oh + kh - 1, ow + kw - 1, ci]
 * x NHWC [N,H,W,Cin] and dz NHWC [N,H,W,Cout] in dtype, dw fp32 in the folded weight's [Cout][3][3][Cin] order;
 * accumulate = 0 overwrites dw, 1 adds to it.  fp32 accumulation in a fixed order: the same call gives the same bits.
 * One implicit-GEMM launch (M = Cout, N = 9 Cin, K = N H W, both operands k-major; csrc/convwgrad.hip) with a
 * deterministic split-K over `workspace` (device, 16-byte aligned, at least
 * sat_conv3x3_wgrad_workspace_bytes(...) bytes for the same shape and policy; the call zeroes its tickets itself).
 * workspace = NULL runs unsplit.  policy->split_k > 0 forces that split count where K has that many 64-pixel
 * k-tiles.  One workspace serves calls ordered on one stream.
 * Shapes: Cin and Cout multiples of 128, any N, H, W >= 1, each tensor under 2 GiB.  Anything else fails with
 * SAT_ERR_INVALID (_workspace_bytes: 0); there is no second path.
 * dtype SAT_F32 (the parity path, not a performance path) gathers the im2col matrix [N H W][9 Cin] into the workspace
 * (required; it must stay under 2 GiB) and runs the exact fp32 sat_gemm product on it. */
size_t sat_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype, const SatPolicy* policy);
int sat_conv3x3_wgrad(int N, int H, int W, int Cin, int Cout, int dtype, const void* x, const void* dz, float* dw,
                      int accumulate, void* workspace, size_t workspace_bytes, const SatPolicy* policy,
                      void* stream);

/* out[i] = y[i] > 0 ? g[i] (+ add[i]) : 0 -- the gradient through a ReLU whose output y was kept (nn.ReLU backward:
 * VGG19's conv + ReLU, encoder.py:24-27, and the three ReLUs of Bottleneck.forward); y NULL = no mask (a plain sum and
 * cast: the identity shortcut's dX = dZ1 W1 + dZ3).  Each tensor in its own dtype (SAT_F32 | SAT_BF16), the sum in
 * fp32, rounded once; 16-byte vectors when every pointer is 16-byte aligned.  out may alias g or add. */
int sat_relu_mask(const void* y, int y_dtype, const void* g, int g_dtype, const void* add, int add_dtype, void* out,
                  int out_dtype, int64_t n, void* stream);
/* The forward fold of one convolution (+ eval-mode BatchNorm, train.py:122) as ONE launch, with the arithmetic of
 * the encoder's plan in its operation order (torchvision conv + bn in eval mode, encoder.py:13-17,24-27):
 *   scale = bn_weight / sqrt(bn_var + eps);  w' = weight * scale;  b' = bn_bias + (bias - bn_mean) * scale
 * (bn_* NULL: w' = weight, b' = bias; bias NULL = 0).  weight: raw fp32 [Cout][Cin][KH][KW].  Writes
 *   w_fold  [Cout][KH][KW][Cin] in dtype, b_fold fp32 [Cout], and (nullable) the input-gradient copy
 *   w_igrad [Cin][KH-1-kh][KW-1-kw][Cout] in dtype: dX = conv(dZ, w_igrad) with the same stride 1 and padding. */
int sat_conv_fold(int Cout, int Cin, int KH, int KW, int dtype, const float* weight, const float* bias,
                  const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                  void* w_fold, float* b_fold, void* w_igrad, void* stream);
/* One trainable convolution of the trunk's tail: its raw fp32 parameters (weight [Cout][Cin][KH][KW]; bias and the
 * BatchNorm tensors nullable), its folded copies (sat_conv_fold) and where its gradients go (fp32, the parameters'
 * shapes; the BN pair required with bn_weight, bias_grad with bias). */
typedef struct {
  const float* weight; const float* bias;
  const float* bn_weight; const float* bn_mean; const float* bn_var; float eps;
  const void* w_fold; const void* w_igrad;
  float* weight_grad; float* bias_grad; float* bn_weight_grad; float* bn_bias_grad;
} SatConvTrain;
/* The fold's chain rule (autograd through eval-mode BatchNorm into the conv, encoder.py:13-17): from the folded
 * gradients dw_fold fp32 [Cout][KH][KW][Cin] and db_fold fp32 [Cout], with s = bn_weight rstd, rstd = 1 / sqrt(var + eps):
 *   weight_grad[co,ci,kh,kw] = dw_fold[co,kh,kw,ci] s[co]
 *   bn_weight_grad[co] = rstd[co] (sum_k dw_fold[co,k] weight[co,k] + db_fold[co] (bias[co] - bn_mean[co]))
 *   bn_bias_grad[co] = db_fold[co];  bias_grad[co] = db_fold[co] s[co]
 * (no BatchNorm: s = 1, so the layout change and bias_grad = db_fold).  One workgroup per output channel, sums in a
 * fixed order.  accumulate = 0 overwrites the gradients, 1 adds to them.  w_fold / w_igrad are not read. */
int sat_conv_fold_backward(int Cout, int Cin, int KH, int KW, const float* dw_fold, const float* db_fold,
                           const SatConvTrain* conv, int accumulate, void* stream);
/* Backward of one identity-shortcut, stride-1 torchvision Bottleneck with eval-mode BatchNorm (Bottleneck.forward
 * through encoder.py:13-17; ResNet152 layer4 blocks 1 and 2) in ONE call; C++ issues the launches:
 *   dZ3 = [y > 0] dy;  dW3' = dZ3^T a2;  dA2 = dZ3 W3';  dZ2 = [a2 > 0] dA2;  dW2' = sat_conv3x3_wgrad(a1, dZ2);
 *   dA1 = conv3x3(dZ2, c2->w_igrad);  dZ1 = [a1 > 0] dA1;  dW1' = dZ1^T x;  dx = dZ1 W1' + dZ3;
 *   db' = column sums of dZ;  each (dW', db') through sat_conv_fold_backward into c1 / c2 / c3's gradients.
 * x, y NHWC [N,H,W,Cin], a1 = relu(c1), a2 = relu(c2) NHWC [N,H,W,Cmid]: the forward's own tensors, in dtype; dy and
 * dx (nullable) [N,H,W,Cin] in dtype.  Gradients handed between layers are rounded once to dtype; weight and bias
 * gradients and every reduction stay fp32, in a fixed order.  Cin and Cmid multiples of 128.  workspace: device,
 * 256-byte aligned, at least _workspace_bytes for the same arguments; one workspace serves calls ordered on one stream. */
size_t sat_bottleneck_backward_workspace_bytes(int N, int H, int W, int Cin, int Cmid, int dtype,
                                               const SatPolicy* policy);
int sat_bottleneck_backward(int N, int H, int W, int Cin, int Cmid, int dtype, const void* x, const void* a1,
                            const void* a2, const void* y, const SatConvTrain* c1, const SatConvTrain* c2,
                            const SatConvTrain* c3, const void* dy, void* dx, int accumulate, void* workspace,
                            size_t workspace_bytes, const SatPolicy* policy, void* stream);
/* Backward of one 3x3 / stride-1 / pad-1 Conv2d + ReLU (VGG19's block-5 units, encoder.py:24-27) in ONE call:
 *   dZ = [y > 0] dy;  dW' = sat_conv3x3_wgrad(x, dZ);  db' = column sums of dZ;  dx = conv3x3(dZ, c->w_igrad);
 * x NHWC [N,H,W,Cin], y and dy [N,H,W,Cout], dx (nullable) [N,H,W,Cin], all in dtype.  Otherwise as
 * sat_bottleneck_backward. */
size_t sat_conv3x3_relu_backward_workspace_bytes(int N, int H, int W, int Cin, int Cout, int dtype,
                                                 const SatPolicy* policy);
int sat_conv3x3_relu_backward(int N, int H, int W, int Cin, int Cout, int dtype, const void* x, const void* y,
                              const SatConvTrain* c, const void* dy, void* dx, int accumulate, void* workspace,
                              size_t workspace_bytes, const SatPolicy* policy, void* stream);

/* --- attention (attention.py:14-21), standalone module forward ----------- */
/* Ws: workspace [B,L,E] fp32. Weights fp32 (U_w [E,E], W_w [E,D], v_w [E]); W_w_lp (bf16 copy)
 * required when dtype == SAT_BF16. context [B,D] fp32, alpha [B,L] fp32. */
int sat_attention_forward(int B, int L, int D, int E, int dtype, const void* img_features,
                          const float* hidden, const float* U_w, const float* U_b,
                          const float* W_w, const void* W_w_lp, const float* W_b,
                          const float* v_w, const float* v_b, float* ws_scratch,
                          float* context, float* alpha, void* stream);


/* --- decoder (decoder.py:69-158) ----------------------------------------- */
/* diagnostics (bench.py): after sat_decoder_forward + sat_decoder_backward filled `workspace`, re-issue
 * each per-step kernel group of step (T-1)/2 `reps` times back to back between HIP events on `stream`;
 * us_out[8] = average us per launch: h GEMM, attention fwd, context GEMM, LSTM fwd, LSTM bwd, d(gated
 * context) GEMM, attention bwd, dh GEMM (0 for groups the configuration does not run).  Overwrites the
 * workspace's running BPTT sums (call after the gradients are consumed). */
int sat_decoder_step_bench(const SatDecoderDims* dims, const SatDecoderLayout* layout, const float* params,
                           const void* params_lp, const void* img_features, void* workspace, size_t workspace_bytes,
                           float* alphas, const float* d_alphas, int reps, float* us_out, void* stream);
size_t sat_decoder_workspace_bytes(const SatDecoderDims* d);
/* The per-step kernel instance a sat_decoder_forward / _backward with these dims (and policy) runs, for tests
 * and bench reports: out[i] for i < n, in this order (SAT_DECODER_INSTANCE_FIELDS values):
 *   0 h-GEMM split-K slabs, 1 context-GEMM slabs, 2 d(gated context) slabs, 3 dh slabs,
 *   4 attention-backward slot chunks per batch row (1 = one workgroup per row, no last-arriver combine;
 *     0 = the two-launch form or no attention), 5 backward products on the transposed weight copies,
 *   6 launches per forward time step, 7 launches per BPTT time step (teacher forcing). */
enum { SAT_DECODER_INSTANCE_FIELDS = 8 };
int sat_decoder_instance(const SatDecoderDims* d, const SatDecoderLayout* lay, int* out, int n);
/* bf16 mode: rewrite the transposed weight copies layout->wih_ctx_t / hcat_t inside params_lp from the shadow's
 * own W_ih / hcat rows (after the shadow changed: the fused Adam step, a cast); a no-op when either is -1. */
int sat_decoder_refresh_transposed(const SatDecoderDims* d, const SatDecoderLayout* lay, void* params_lp,
                                   void* stream);
/* preds [B,T-1,V] (dtype), alphas [B,T-1,L] fp32, tokens [B,T-1] int32 = token fed at each step. */
int sat_decoder_forward(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                        const void* params_lp, const void* img_features, const int64_t* captions,
                        const uint8_t* dropout_mask, void* workspace, size_t workspace_bytes,
                        void* preds, float* alphas, int32_t* tokens, void* stream);
/* Scheduled sampling (Bengio et al. 2015): sat_decoder_forward with the fed token chosen per row and step between
 * the reference's two modes -- the ground-truth token (decoder.py:108-112) and the previous step's argmax
 * (decoder.py:131-133).  Step 0 feeds the start token; at step t >= 1 row b feeds captions[b, t] where keep[b, t] = 1
 * (an id outside [0, V) is clamped to 0, as the argmax id is) and argmax(preds[b, t-1]) (first index on ties) elsewhere.
 *   keep = tf_mask[b, t] != 0 when tf_mask ([B, T-1] uint8, column 0 ignored) is given; otherwise the draw
 *   u(seed, b, t) < p with u in [0, 1), p = *tf_prob_dev when tf_prob_dev is given (a device scalar read by the
 *   kernels, so a captured graph follows a schedule) and tf_prob otherwise: p = 1 keeps every position, p = 0 none.
 * The draw takes the dropout's seed (d->seed ^ f(*d->seed_ptr), the counter advanced once per training forward) under
 * a domain constant of its own, and depends on (seed, b, t) only.  tf_mask_out (nullable, [B, T-1] uint8) receives
 * the keep bits used, column 0 as 1.  Requires d->tf == 0 and 0 <= tf_prob <= 1 (SAT_ERR_INVALID otherwise); the
 * workspace is that of d (tf == 0) and sat_decoder_backward runs on it unchanged: the fed tokens are constants. */
int sat_decoder_forward_sampled(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                                const void* params_lp, const void* img_features, const int64_t* captions,
                                const uint8_t* dropout_mask, float tf_prob, const float* tf_prob_dev,
                                const uint8_t* tf_mask, uint8_t* tf_mask_out, void* workspace,
                                size_t workspace_bytes, void* preds, float* alphas, int32_t* tokens, void* stream);
/* Sampled feedback (the sample pass of self-critical sequence training, Rennie et al. 2017): sat_decoder_forward
 * with the decoder drawing its next token from its own distribution.  Step 0 feeds the start token, step t >= 1
 * feeds sampled[b, t-1], and a token is drawn at every step, the last included:
 *   sampled[b, t] = argmax_v ( x[b,t,v] + tau * G(seed, b, t, v) )
 * x = the stored logits of preds (bf16: the rounded values; ado: after the ReLU -- what the greedy argmax reads), the
 * sum formed in fp32 as one multiply then one add (no contraction), the winner taken in torch.argmax's order (NaN
 * first, then the value, then the smaller index).  This is the Gumbel-max form of a draw from softmax(x / tau): no
 * division, tau = 0 is the greedy forward bit for bit, a logit of -inf is never drawn.
 *   G = -log(-log u), u = (2k + 1) 2^-24, k = the top 23 bits of the 64-bit mix of scheduled sampling's draw taken over
 *   (seed, b, t, v) under a domain constant of its own: u is exact in fp32 and never 0 or 1, so G is finite.  The seed
 *   is the dropout's (d->seed ^ f(*d->seed_ptr)); the counter is advanced once per sample-mode forward (training or
 *   not), so a captured graph draws afresh on every replay.  G depends on (seed, b, t, v) only, not on the loop form.
 * tau = *temperature_dev when temperature_dev is given (a device scalar read by the kernels), temperature otherwise.
 * Requires d->tf == 0, temperature >= 0 (NaN refused) and V < 2^20 (SAT_ERR_INVALID otherwise).  captions is
 * nullable and unread (d->T and d->start_token define the steps).  tokens (nullable, [B, T-1]) receives the fed
 * tokens, sampled ([B, T-1] int32) the drawn ones.  The workspace is that of d (tf == 0) and sat_decoder_backward runs
 * on it unchanged: the fed tokens are constants. */
int sat_decoder_forward_sample(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                               const void* params_lp, const void* img_features, const int64_t* captions,
                               const uint8_t* dropout_mask, float temperature, const float* temperature_dev,
                               void* workspace, size_t workspace_bytes, void* preds, float* alphas, int32_t* tokens,
                               int32_t* sampled, void* stream);
/* diagnostic: out[b, t, v] ([B, T1, V] fp32) = exactly the G values the next sample-mode forward of d will use (the
 * same device function; only d->seed and d->seed_ptr are read).  Does not advance the counter. */
int sat_sample_noise(const SatDecoderDims* d, int B, int T1, int V, float* out, void* stream);
/* phase 1 = output-head gradients only (f_out/f_h/f_z/deep_output), 2 = the rest
 * (needs phase 1 first), 3 = both.  accumulate=0 overwrites the active grads. */
int sat_decoder_backward(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                         const void* params_lp, const void* img_features, void* workspace,
                         size_t workspace_bytes, const void* preds, const float* alphas,
                         const void* d_preds, const float* d_alphas, float* grads, int accumulate,
                         int phase, void* stream);   /* phase 1 | 2 | 3, + 4: d_preds already ReLU-masked (ado),
                                                     + 8: d_preds rows zero-padded to the bf16 head's
                                                     stride (sat_caption_loss_backward_ld; ado needs 4) */
/* sat_decoder_backward that also returns dL/d(img_features) -- what loss.backward() leaves in the reference's
 * encoder output (encoder.py:13-17 never freezes it; attention.py:14-21, decoder.py:101-105,137-147):
 *   d_features[b,l,:] = sum_t alpha[b,t,l] dL/dcontext_t[b,:]            (the context, attention.py:19-20)
 *                     + (dL/dWs . attention.W.weight)[b,l,:]             (the attention projection, attention.py:16)
 *                     + (dL/d[init_h | init_c pre-activations] . [init_h.weight; init_c.weight])[b,:] / L
 * (without attention the first two are sum_t (d gates_t . W_ih[:, E:] + d f_z,t . f_z.weight)[b,:] / L).
 * d_features: [B,L,D] in the features' dtype, overwritten (never accumulated into) by the call's phase 2 and left
 * untouched by a phase-1-only call; fg_workspace: sat_decoder_feature_grad_workspace_bytes(d) bytes, 16-byte
 * aligned, used by phase 2 only (it needs no content from phase 1 or the forward).  With d_features == NULL the
 * call is exactly sat_decoder_backward (fg_workspace is ignored).  Capturable like every other entry. */
int sat_decoder_backward_features(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                                  const void* params_lp, const void* img_features, void* workspace,
                                  size_t workspace_bytes, const void* preds, const float* alphas,
                                  const void* d_preds, const float* d_alphas, float* grads, int accumulate,
                                  int phase, void* stream, void* d_features, void* fg_workspace,
                                  size_t fg_workspace_bytes);
/* bytes of sat_decoder_backward_features' fg_workspace (every step's dL/dcontext [B (T-1), D] fp32, the fp32
 * attention.W product [B L, D], the init product [B, D]); 0 for unsupported dims.  sat_decoder_workspace_bytes
 * is unaffected. */
size_t sat_decoder_feature_grad_workspace_bytes(const SatDecoderDims* d);
/* The accumulation kernel of the above on its own:
 *   out[b,l,:] = sum_{t < T1} alpha[b,t,l] dctx[b,t,:] + mean_term[b,:] / L + addend[b,l,:]
 * summed in fp32 in step order and rounded once to dtype (SAT_F32 / SAT_BF16).  Element strides: alpha[b,t,l] at
 * b alpha_stride_b + t alpha_stride_t + l; dctx[b,t,:] at b dctx_stride_b + t dctx_stride_t; rows b L + l of
 * addend / out at addend_ld / out_ld; row b of mean_term at mean_ld.  addend and mean_term are nullable.
 * D % 8 == 0, 1 <= L <= 1024, T1 >= 1, 16-byte aligned rows (fp32 strides multiples of 4, out_ld of 16 bytes). */
int sat_feature_grad_accumulate(int B, int L, int D, int T1, int dtype, const float* alpha, int64_t alpha_stride_b,
                                int64_t alpha_stride_t, const float* dctx, int64_t dctx_stride_b,
                                int64_t dctx_stride_t, const float* addend, int64_t addend_ld,
                                const float* mean_term, int64_t mean_ld, void* out, int64_t out_ld, void* stream);

/* --- beam-search captioning (decoder.py:160-269, Decoder.caption; generate_caption.py:86-88) ---
 * img_features: DEVICE [beam_size, L, D] (the reference expands one image to beam rows).
 * Uses d->L, D, E, V, ado, attention, bert, dtype, start_token; d->B, T, tf, training are ignored
 * (caption() applies no dropout).  Runs up to max_step + 1 decoder steps (the reference: 50),
 * synchronising `stream` once per step to retire/compact beams, so it is NOT capturable.
 * Results are written to HOST memory:
 *   out_ids    [max_step + 2]        best completed sentence incl. the start token
 *   out_alphas [(max_step + 2) * L]  its alpha rows (first row = ones, as in decoder.py:173)
 *   out_score                        its summed raw logits; -inf when no beam completed, in which
 *                                    case out_ids = [0] and out_alphas holds the last step's
 *                                    *out_alpha_rows alpha rows (decoder.py:256-258).
 * Requires 1 <= beam_size <= min(64, max_step + 2). */
size_t sat_decoder_beam_workspace_bytes(const SatDecoderDims* d, int beam_size);
int sat_decoder_beam_search(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                            const void* params_lp, const void* img_features, int beam_size, int max_step,
                            void* workspace, size_t workspace_bytes, int32_t* out_ids, int* out_len,
                            float* out_alphas, int* out_alpha_rows, float* out_score, void* stream);

/* --- batched beam search: n_images images x beam_size beams decoded together --------------------------
 * Per image exactly sat_decoder_beam_search's result (same candidate order, end ids, winner rule and
 * no-completion case), but every launch carries n_images * beam_size rows and the top-k selection,
 * end-token retirement, survivor reordering, histories and the final backtrack all run on the device.
 * img_features: DEVICE [n_images, L, D], one row block per image, NOT expanded to beam rows.
 * The step loop issues no copy and no synchronise except a 4-byte early-exit poll every 8th step; one
 * synchronise follows the final copies, so `stream` is idle on return (NOT capturable).
 * Results are written to HOST memory, image n at:
 *   out_ids        + n * (max_step + 2)        sentence incl. the start token, out_len[n] ids
 *   out_alphas     + n * (max_step + 2) * L    out_alpha_rows[n] alpha rows (first row = ones)
 *   out_score[n]                               summed raw logits; -inf when no beam of the image completed:
 *                                              then ids = [0], len = 1 and the alpha rows are the last
 *                                              step's live rows.
 * Requires n_images >= 1, 1 <= beam_size <= min(64, max_step + 2), n_images * beam_size <= 1024 and the
 * dims sat_decoder_beam_search accepts; otherwise SAT_ERR_INVALID / 0 bytes.  The workspace holds the
 * alpha history: (max_step + 1) * n_images * beam_size * L floats on top of the per-row step buffers. */
size_t sat_decoder_beam_batch_workspace_bytes(const SatDecoderDims* d, int n_images, int beam_size, int max_step);
int sat_decoder_beam_search_batch(const SatDecoderDims* d, const SatDecoderLayout* lay, const float* params,
                                  const void* params_lp, const void* img_features, int n_images, int beam_size,
                                  int max_step, void* workspace, size_t workspace_bytes, int32_t* out_ids,
                                  int* out_len, float* out_alphas, int* out_alpha_rows, float* out_score,
                                  void* stream);

/* --- loss + metrics (train.py:135-162, utils.py:44-80,101-107) ----------- */
size_t sat_caption_loss_workspace_bytes(int B, int T, int L);
/* out[0]=loss, [1]=CE, [2]=att-reg, [3]=#top1-correct, [4]=#top5-correct, [5]=#non-pad targets,
 * [6]=caption length (tokens not in skip_ids). */
int sat_caption_loss_forward(int B, int T, int V, int L, int dtype, const void* preds,
                             const float* alphas, const int64_t* captions, float alpha_c,
                             int pad_id, int skip0, int skip1, int skip2, void* workspace,
                             float* out, void* stream);
/* the same, the loss (out[0]) also written to loss_out (its own 4-byte buffer: the autograd wrapper hands it out
 * as a tensor a caller may scale in place, without a device copy of out[0]) */
int sat_caption_loss_forward_loss_out(int B, int T, int V, int L, int dtype, const void* preds,
                                      const float* alphas, const int64_t* captions, float alpha_c,
                                      int pad_id, int skip0, int skip1, int skip2, void* workspace,
                                      float* out, float* loss_out, void* stream);
int sat_caption_loss_backward(int B, int T, int V, int L, int dtype, const void* preds,
                              const int64_t* captions, float alpha_c, void* workspace,
                              const float* grad_out, void* d_preds, float* d_alphas, void* stream);
/* the same with the logits a ReLU's output (decoder.py:117-125 advanced deep output): the gradient
 * leaves through that ReLU (zero where preds <= 0), so the decoder backward can skip its mask pass
 * (sat_decoder_backward phase bit 4). */
int sat_caption_loss_backward_relu(int B, int T, int V, int L, int dtype, const void* preds,
                              const int64_t* captions, float alpha_c, void* workspace,
                              const float* grad_out, void* d_preds, float* d_alphas, void* stream);
/* either of the two with d_preds rows ld_dpreds >= V elements apart and columns V..ld_dpreds-1
 * written as zeros (relu_mask != 0: the _relu form).  The bf16 decoder head pads odd vocabularies
 * to a multiple of 8 (16-B rows, e.g. BERT's 30522 -> 30528); a gradient handed over in that
 * layout skips the decoder's copy into padded rows (sat_decoder_backward phase bit 8). */
int sat_caption_loss_backward_ld(int B, int T, int V, int L, int dtype, const void* preds,
                                 const int64_t* captions, float alpha_c, void* workspace,
                                 const float* grad_out, void* d_preds, int64_t ld_dpreds,
                                 float* d_alphas, int relu_mask, void* stream);
/* Token-weighted caption loss (self-critical sequence training's reward-weighted log-likelihood):
 *   loss = sum_{b, t < T-1} w[b,t] (logsumexp(preds[b,t,:]) - preds[b,t,target[b,t]])
 *          + alpha_c * mean_{b,l} (1 - sum_t alpha[b,t,l])^2
 *   d preds[b,t,:] = g * w[b,t] * (softmax(preds[b,t,:]) - onehot(target[b,t]))
 * targets [B,T-1] int32 and weights [B,T-1] fp32 are device arrays; all T-1 steps are eligible, the weights decide
 * what is scored.  A row with w == 0 gets an exactly zero gradient row and its logits are not read by the backward.
 * A target outside [0, V) cannot be refused without a host read: such a row counts as weight 0 (loss, gradient) and
 * is tallied in out[3]; its logp is 0.  Reductions run in a fixed order (bit-identical reruns).
 * forward: out[0] = loss, [1] = the weighted CE sum, [2] = att-reg, [3] = # out-of-range targets (out: >= 4 floats);
 * loss_out (its own 4-byte buffer) = out[0]; logp[b,t] = preds[b,t,target] - logsumexp, fp32 [B,T-1].
 * backward: the workspace of the forward; ld_dpreds / relu_mask as sat_caption_loss_backward_ld's. */
size_t sat_caption_loss_weighted_workspace_bytes(int B, int T, int L);
int sat_caption_loss_weighted_forward(int B, int T, int V, int L, int dtype, const void* preds,
                                      const float* alphas, const int32_t* targets, const float* weights,
                                      float alpha_c, void* workspace, float* out, float* loss_out, float* logp,
                                      void* stream);
int sat_caption_loss_weighted_backward(int B, int T, int V, int L, int dtype, const void* preds,
                                       const int32_t* targets, const float* weights, void* workspace,
                                       const float* grad_out, void* d_preds, int64_t ld_dpreds, float* d_alphas,
                                       int relu_mask, void* stream);

/* --- streaming image input (train.py:27-32 transform, dataset.py:9-12 decode on the host) ------
 * Decoded uint8 RGB images of any size, packed HWC (image b at pixels + offsets[b], sizes[b] =
 * {H, W}; offsets / sizes are device arrays) -> Resize((OH, OW)) with Pillow's 8-bit BILINEAR
 * resampler (bit-identical bytes) -> ToTensor -> Normalize(mean, std) (host float[3] each) -> the
 * encoder's input layout.  max_h / max_w bound the sizes (downscale <= sat_images_max_downscale()).
 * One workgroup needs sat_images_lds_bytes(max_h, max_w, OH, OW) bytes of LDS (0 for a non-positive size); a batch
 * that needs more than sat_images_lds_limit() -- the device's per-workgroup LDS, 160 KiB on gfx950; only outputs
 * near 512 columns at a 13x or deeper horizontal downscale do -- is SAT_ERR_INVALID before any launch. */
enum { SAT_IMG_NCHW = 0, SAT_IMG_NHWC = 1, SAT_IMG_S2D16 = 2 };
size_t sat_images_workspace_bytes(int B, int OH, int OW);
int sat_images_max_downscale(void);
size_t sat_images_lds_bytes(int max_h, int max_w, int OH, int OW);
size_t sat_images_lds_limit(void);
int sat_images_to_input(const uint8_t* pixels, const int64_t* offsets, const int32_t* sizes, int B, int max_h,
                        int max_w, int OH, int OW, const float* mean, const float* std, int layout, int c_pad,
                        int dtype, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* --- row gather / scatter against a device-resident table (the feature cache: the frozen trunk's output per image,
 * computed once and kept in HBM instead of re-encoding dataset.py's repeated image per caption) ----
 *   sat_rows_gather :  out[i, :]        = table[idx[i], :]   for i < n
 *   sat_rows_scatter:  table[idx[i], :] = src[i, :]          for i < n  (idx distinct: rows of equal index race)
 * table is [n_rows, row_elems], out / src [n, row_elems], all contiguous, dtype SAT_BF16 or SAT_F32; idx is a DEVICE
 * array read by the kernel, so a captured launch follows a rewritten index buffer.  An index outside [0, n_rows)
 * makes the gather write a zero row and the scatter skip the row; each such row adds 1 to *n_bad (device, nullable,
 * zeroed by the caller).  Nothing but out, or the addressed table rows, is written.  Rows move as 16-B vectors when
 * the row bytes and both base pointers are 16-B aligned, else element by element; every address is 64-bit (a table
 * may exceed 2^32 bytes).  Null table / src / idx / out, n < 0, n_rows <= 0, row_elems <= 0 or another dtype:
 * SAT_ERR_INVALID before any launch; n == 0 is a successful no-op. */
int sat_rows_gather(const void* table, int64_t n_rows, int64_t row_elems, int dtype, const int64_t* idx, int n,
                    void* out, int32_t* n_bad, void* stream);
int sat_rows_scatter(const void* src, int n, int64_t row_elems, int dtype, const int64_t* idx, void* table,
                     int64_t n_rows, int32_t* n_bad, void* stream);

/* --- CIDEr-D on the device (the reward of self-critical sequence training; the arithmetic of sat_amd/cider.py) ----
 * The corpus is resident, built once, all device arrays:
 *   table          slots x 4 uint32 (16-B aligned, zeroed by the caller before the first insert): an open-addressed
 *                  hash table from n-gram to idf = log N - log max(1, df), fp32.  A slot is the 96-bit key and the
 *                  value; slots in [2, 2^31), any number (not only powers of two), at least one left empty.
 *   key            3 uint32 per n-gram (ids g0..g(n-1), each below 2^20, n = 1..4, the ids past n zero):
 *                    word 0 = n << 20 | g0,  word 1 = g1 | (g2 & 0xfff) << 20,  word 2 = g2 >> 12 | g3 << 8
 *                  The key holds the whole n-gram and n: a hash collision costs a probe, never a value.
 *   ref_words      int32 [n_refs, ref_stride] the stripped reference sentences, ref_len[n_refs] their lengths
 *   img_ref_begin  int32 [n_images + 1]: image i owns references img_ref_begin[i] .. img_ref_begin[i + 1] - 1
 *   ref_norm       float [n_refs, 4]: the norm of every reference's tf-idf vector per n
 * A key absent from the table has df 0 and idf log_n.  Every probe loop ends after `slots` probes.
 *
 * sat_cider_table_insert: stores n keys with their values.  The keys are unique among themselves and against the
 *   table's contents (they come from one document-frequency dictionary); lookups belong in later launches.  A key that
 *   finds no empty slot, or whose word 0 is 0, adds 1 to *n_bad (device, nullable, zeroed by the caller).
 * sat_cider_lookup: out[i] = the value stored under keys[3 i .. 3 i + 2], log_n for an absent key (a diagnostic, and
 *   the lookup the two kernels below use).
 * sat_cider_ref_norms: fills ref_norm from ref_words / ref_len with the scorer's own counting and lookup code.
 * sat_cider_score: out[i] = CIDEr-D of tokens[i, 0 .. T1) against the references of image[i]: start and pad ids are
 *   dropped wherever they stand and the sentence ends before the first end id; sigma = 6, the mean over n = 1..4 and
 *   over the references, times 10; an empty sentence or an image without references scores 0.  One wave per row; a
 *   row's score depends on that row only and reductions run in a fixed order (bit-identical reruns).  tokens
 *   [n, T1] int32, image [n] int64 and out [n] are read and written on the device when the launch runs: the call is
 *   capturable.  An image index outside [0, n_images) scores 0 and adds 1 to *n_bad (device, nullable); a token
 *   outside [0, 2^20) is a word no reference has.
 * T1 or ref_stride outside [1, 64], slots outside [2, 2^31), a table not 16-B aligned, a null array or a negative
 * count: SAT_ERR_INVALID before any launch; n == 0 (n_refs == 0 for the norms) is a successful no-op. */
int sat_cider_table_insert(uint32_t* table, int64_t slots, const uint32_t* keys, const float* values, int64_t n,
                           int32_t* n_bad, void* stream);
int sat_cider_lookup(const uint32_t* table, int64_t slots, float log_n, const uint32_t* keys, int64_t n, float* out,
                     void* stream);
int sat_cider_ref_norms(const uint32_t* table, int64_t slots, float log_n, const int32_t* ref_words,
                        const int32_t* ref_len, int n_refs, int ref_stride, float* ref_norm, void* stream);
int sat_cider_score(const uint32_t* table, int64_t slots, float log_n, const int32_t* ref_words,
                    const int32_t* ref_len, const float* ref_norm, int n_refs, int ref_stride,
                    const int32_t* img_ref_begin, int n_images, const int32_t* tokens, const int64_t* image, int n,
                    int T1, int start_id, int end_id, int pad_id, float* out, int32_t* n_bad, void* stream);

/* --- optimiser (torch.optim.Adam single-tensor step, train.py:71,164) ---- */
int sat_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  void* param_lp, int64_t n, float beta1, float beta2, float eps,
                  float step_size, float bias_correction2_sqrt, void* stream);

/* --- gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, L2) ---
 * Three launches ordered by the stream alone: the partials of every gradient range, one finalize, then the update.
 * No atomics, no host read; every sum is fp64 in a fixed order, so the norm is identical from run to run.
 * grad_sumsq: one 256-thread workgroup per partial; workgroup i writes partials[i], the fp64 sum of squares of its
 *   share of g[0..n) (16-B loads where g is 16-B aligned, scalars for the head and tail), 0 where the share is empty.
 *   g needs 4-byte, partials 8-byte alignment.
 * grad_clip_finalize: adds partials[0..n) and writes state[0] = norm (fp32), state[1] = scale =
 *   min(1, max_norm / (norm + 1e-6)), state[2] = 1 when the total is not finite (then scale = 0), else 0, and adds
 *   state[2] to state[3], the count of skipped steps.  state: 4 floats on the device, zeroed once by the caller.
 * adam_step_scaled: sat_adam_step on grad[i] * state[1] (the product rounded to fp32 first: the same bits as
 *   sat_adam_step on pre-scaled gradients); when state[2] != 0 it leaves param, both moments and param_lp untouched. */
int sat_grad_sumsq(const float* g, int64_t n, double* partials, int n_partials, void* stream);
int sat_grad_clip_finalize(const double* partials, int n, float max_norm, float* state, void* stream);
int sat_adam_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                         void* param_lp, int64_t n, float beta1, float beta2, float eps,
                         float step_size, float bias_correction2_sqrt, const float* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAT_HIP_H_ */

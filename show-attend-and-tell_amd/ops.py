"""Tensor-level wrappers over the C ABI (shape checks, output allocation, stream).

Every function here launches HIP kernels on the tensors' current stream and
never falls back to a PyTorch compute op.
"""
import ctypes

import torch

from . import _lib as L


def linear(x, weight, bias=None, act=L.ACT_NONE, out_dtype=None, weight_lp=None):
    """y = act(x @ weight.T + bias) on MFMA (nn.Linear forward).  x [M,K] (f32|bf16),
    weight [N,K] f32 (or weight_lp bf16 when x is bf16)."""
    L.require_device(x, weight)
    M, K = x.shape
    N = weight.shape[0]
    dt = L.dtype_code(x.dtype)
    if dt == L.SAT_F32:
        w = weight
    elif weight_lp is not None:
        w = weight_lp
    else:
        w = cast_(weight.contiguous(), torch.empty(weight.shape, device=weight.device, dtype=torch.bfloat16))
    out_dtype = out_dtype or torch.float32
    y = torch.empty(M, N, device=x.device, dtype=out_dtype)
    gemm(x, w, y, bias=bias, act=act)
    return y


_GEMM_WS = {}


def gemm_workspace(device, stream):
    """The split-K workspace sat_gemm may use (include/sat_hip.h SatGemmArgs.workspace), one per device and stream:
    calls ordered on one stream share it.

    The split kernel's arrival tickets and partial tiles live in the workspace, so two launches that may run at the
    same time must not share one.  Under stream capture the current stream is torch's shared capture stream, and
    graphs captured on it could be replayed concurrently on different streams: during a capture every call gets a
    workspace of its own (allocated in the graph's private pool, alive as long as the graph's pool).  Graphs that use
    ``gemm`` on the cached workspace (eager calls) are therefore never tied to each other."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(int(L.lib().sat_gemm_workspace_bytes()), dtype=torch.uint8, device=device)
    key = (torch.device(device).index, stream.value or 0)
    ws = _GEMM_WS.get(key)
    if ws is None:
        ws = torch.empty(int(L.lib().sat_gemm_workspace_bytes()), dtype=torch.uint8, device=device)
        _GEMM_WS[key] = ws
    return ws


def _may_split(A, C, bias, aux, act, K):
    """Whether sat_gemm could take the split-K path for this call (csrc/gemmsplit.hip split_eligible): bf16 operands,
    an fp32 C, no bias / aux / activation epilogue and a long K.  Other calls never touch a workspace."""
    return (A.dtype == torch.bfloat16 and C.dtype == torch.float32 and bias is None and aux is None
            and act == L.ACT_NONE and K >= 512)


def gemm(A, B, C, *, transA=False, transB=False, alpha=1.0, beta=0.0, bias=None, add1=None, act=L.ACT_NONE,
         aux=None, policy=None, workspace=True):
    """C = act(alpha * A' B'^T + bias + add1 + beta*C) with A' = A or A^T, B'(n,k) = B[n,k] or B[k,n].
    ``policy``: an optional ``sat_amd.Policy`` (per-call kernel selection; None = library defaults).
    ``workspace``: True = this stream's cached split-K workspace (``gemm_workspace``), a uint8 device tensor, or
    None (products with fp32 output and a k-major operand then run unsplit)."""
    a = _gemm_args(A, B, C, transA, transB, alpha, beta, bias, add1, act, aux, policy)
    stream = L.stream_of(C)
    if workspace is True:
        workspace = (gemm_workspace(C.device, stream)
                     if policy is not None or _may_split(A, C, bias, aux, act, a.K) else None)
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    L.check(L.lib().sat_gemm(ctypes.byref(a), stream), "sat_gemm")
    return C


def _gemm_args(A, B, C, transA=False, transB=False, alpha=1.0, beta=0.0, bias=None, add1=None, act=L.ACT_NONE,
               aux=None, policy=None):
    L.require_device(A, B, C)
    dt = L.dtype_code(A.dtype)
    if B.dtype != A.dtype:
        raise TypeError("sat_amd.gemm: A and B must share a dtype")
    M = A.shape[1] if transA else A.shape[0]
    K = A.shape[0] if transA else A.shape[1]
    N = B.shape[1] if transB else B.shape[0]
    Kb = B.shape[0] if transB else B.shape[1]
    if Kb != K or C.shape[0] != M or C.shape[1] != N:
        raise ValueError(f"sat_amd.gemm: shape mismatch A{tuple(A.shape)} B{tuple(B.shape)} C{tuple(C.shape)}")
    for t in (A, B, C, add1, aux):
        if t is not None and t.stride(-1) != 1:
            raise ValueError("sat_amd.gemm: operands must be row-major with unit inner stride")
    a = L.SatGemmArgs()
    a.M, a.N, a.K, a.dtype = M, N, K, dt
    a.A, a.lda, a.transA = A.data_ptr(), A.stride(0), int(transA)
    a.B, a.ldb, a.transB = B.data_ptr(), B.stride(0), int(transB)
    a.C, a.ldc, a.c_dtype = C.data_ptr(), C.stride(0), L.dtype_code(C.dtype)
    a.alpha, a.beta = alpha, beta
    a.bias = bias.data_ptr() if bias is not None else None
    if add1 is not None:
        a.add1, a.ld_add1, a.add1_dtype = add1.data_ptr(), add1.stride(0), L.dtype_code(add1.dtype)
    a.act = act
    if aux is not None:
        a.aux, a.ld_aux, a.aux_dtype = aux.data_ptr(), aux.stride(0), L.dtype_code(aux.dtype)
    a.policy = L.policy_ptr(policy)
    return a


def gemm_group(products, workspace):
    """Independent products as one launch (include/sat_hip.h sat_gemm_group).  ``products``: up to 8 dicts of
    ``gemm``'s arguments (A, B, C and the keywords but ``workspace``), each with its own ``policy``; ``workspace``: a
    uint8 device tensor of at least ``sat_gemm_group_workspace_bytes()``, which the call may overwrite."""
    args = (L.SatGemmArgs * len(products))()
    keep = []
    for i, p in enumerate(products):
        a = _gemm_args(**p)
        keep.append(a)   # the policy pointers stay alive until the call returns
        ctypes.memmove(ctypes.byref(args[i]), ctypes.byref(a), ctypes.sizeof(a))
    L.check(L.lib().sat_gemm_group(args, len(products), workspace.data_ptr(),
                                   workspace.numel() * workspace.element_size(), L.stream_of(products[0]["C"])),
            "sat_gemm_group")


def gemm_group_plan(shapes, slab_bytes, tickets):
    """The joint planner of a group launch, on the host (include/sat_hip.h sat_gemm_group_plan).  ``shapes``: tuples
    (M, N, K[, tile_rows[, splits]]); returns one ``SatGemmGroupPlan`` per product."""
    sh = (L.SatGemmGroupShape * len(shapes))()
    for i, t in enumerate(shapes):
        t = tuple(t) + (0, 0)
        sh[i].M, sh[i].N, sh[i].K, sh[i].tile_rows, sh[i].splits = t[:5]
    plan = (L.SatGemmGroupPlan * len(shapes))()
    L.check(L.lib().sat_gemm_group_plan(sh, len(shapes), slab_bytes, tickets, plan), "sat_gemm_group_plan")
    return plan


def gemm_group_block(plan, block):
    """(product, m-tile, n-tile, split) of a block of a planned group launch; product -1 = no such block."""
    out = [ctypes.c_int() for _ in range(4)]
    L.check(L.lib().sat_gemm_group_block(plan, len(plan), block, *[ctypes.byref(o) for o in out]),
            "sat_gemm_group_block")
    return tuple(o.value for o in out)


def cast_(src, dst):
    """dst.copy_(src) between float32/bfloat16 storage, on the HIP path."""
    L.require_device(src, dst)
    assert src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
    L.check(L.lib().sat_cast(L.ptr(src), L.dtype_code(src.dtype), L.ptr(dst), L.dtype_code(dst.dtype),
                             src.numel(), L.stream_of(dst)), "sat_cast")
    return dst


def nchw_to_nhwc(x, c_pad, dtype):
    """[N,C,H,W] f32 -> [N,H,W,c_pad] (dtype), zero-padded channels."""
    L.require_device(x)
    x = x.contiguous() if not x.is_contiguous() else x
    if x.dtype != torch.float32:
        raise TypeError("images must be float32 (post-Normalize domain, train.py:27-32)")
    N, C, H, W = x.shape
    y = torch.empty(N, H, W, c_pad, device=x.device, dtype=dtype)
    L.check(L.lib().sat_nchw_to_nhwc(N, C, H, W, c_pad, L.dtype_code(dtype), L.ptr(x), L.ptr(y), L.stream_of(y)),
            "sat_nchw_to_nhwc")
    return y


def nchw_to_s2d(x, dtype):
    """[N,C,H,W] f32 (C <= 4, H, W even) -> space-to-depth [N,H/2,W/2,16] (dtype)."""
    L.require_device(x)
    x = x.contiguous() if not x.is_contiguous() else x
    if x.dtype != torch.float32:
        raise TypeError("images must be float32 (post-Normalize domain, train.py:27-32)")
    N, C, H, W = x.shape
    y = torch.empty(N, H // 2, W // 2, 16, device=x.device, dtype=dtype)
    L.check(L.lib().sat_nchw_to_s2d(N, C, H, W, L.dtype_code(dtype), L.ptr(x), L.ptr(y), L.stream_of(y)),
            "sat_nchw_to_s2d")
    return y


# Normalize(mean, std) of the reference's transform (train.py:27-32), as float32
IMAGE_MEAN = (0.485, 0.456, 0.406)
IMAGE_STD = (0.229, 0.224, 0.225)


def images_to_input(packed, layout=L.IMG_NCHW, dtype=torch.float32, c_pad=8, size=(224, 224),
                    mean=IMAGE_MEAN, std=IMAGE_STD):
    """Decoded uint8 images (a device-resident ``data.PackedImages``) -> the reference's
    Resize(size) + ToTensor + Normalize(mean, std), bit-identical to PIL + torch, written straight
    into ``layout``: IMG_NCHW [B,3,H,W] f32, IMG_NHWC [B,H,W,c_pad] (dtype) or IMG_S2D16
    [B,H/2,W/2,16] (dtype)."""
    L.require_device(packed.pixels, packed.offsets, packed.sizes)
    lib = L.lib()
    B = packed.count
    OH, OW = size
    mx = lib.sat_images_max_downscale()
    if packed.max_h > mx * OH or packed.max_w > mx * OW:
        raise ValueError(f"images_to_input: {packed.max_h}x{packed.max_w} exceeds the {mx}x downscale limit "
                         f"to {OH}x{OW}")
    need, limit = lib.sat_images_lds_bytes(packed.max_h, packed.max_w, OH, OW), lib.sat_images_lds_limit()
    if need > limit:
        raise ValueError(f"images_to_input: {packed.max_h}x{packed.max_w} to {OH}x{OW} needs {need} bytes of LDS per "
                         f"workgroup, above the limit of {limit}")
    dev = packed.pixels.device
    if layout == L.IMG_NCHW:
        if dtype != torch.float32:
            raise TypeError("images_to_input: the NCHW layout is the reference's float32 tensor")
        out = torch.empty(B, 3, OH, OW, device=dev, dtype=torch.float32)
    elif layout == L.IMG_NHWC:
        out = torch.empty(B, OH, OW, c_pad, device=dev, dtype=dtype)
    elif layout == L.IMG_S2D16:
        out = torch.empty(B, OH // 2, OW // 2, 16, device=dev, dtype=dtype)
    else:
        raise ValueError(f"images_to_input: unknown layout {layout}")
    ws_bytes = lib.sat_images_workspace_bytes(B, OH, OW)
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    m = (ctypes.c_float * 3)(*mean)
    sd = (ctypes.c_float * 3)(*std)
    L.check(lib.sat_images_to_input(L.ptr(packed.pixels), L.ptr(packed.offsets), L.ptr(packed.sizes), B,
                                    packed.max_h, packed.max_w, OH, OW, m, sd, layout, c_pad, L.dtype_code(dtype),
                                    L.ptr(out), L.ptr(ws), ws_bytes, L.stream_of(out)), "sat_images_to_input")
    return out


class ProjectedResidual:
    """The residual of a stage's first bottleneck, not yet computed: the block input ``x`` [B,H,W,Kp] and the folded
    downsample conv ``f`` = (w [N,1,1,Kp], bias f32, stride, pad 0) as the Encoder plan holds it.  conv2d_nhwc and
    conv1x1_chain take it as ``residual=``: the c3 launch then forms the downsample output in registers
    (sat_conv1x1_proj) where conv1x1_proj_supported, else the downsample conv is launched first -- the same bits."""

    def __init__(self, x, f):
        self.x, self.f = x, f

    def out_hw(self):
        s = self.f[2]
        return (self.x.shape[1] - 1) // s + 1, (self.x.shape[2] - 1) // s + 1

    def materialize(self, policy=None):
        """The downsample conv as a launch of its own."""
        return conv2d_nhwc(self.x, *self.f, False, policy=policy)


def conv1x1_proj_supported(M, K, N, Kp, stride, N2, dtype, policy=None):
    """True when the c3 (M pixels, K -> N channels) with a projected residual (Kp -> N channels at ``stride``), chained
    into an N -> N2 c1 when N2 > 0, runs as ONE launch under ``policy``."""
    return bool(L.lib().sat_conv1x1_proj_supported(M, K, N, Kp, stride, N2, L.dtype_code(dtype), L.policy_ptr(policy)))


def _proj_launch(x, c3, proj, c1_next, policy):
    """(y, x1 or None) from the projection kernel, or None where it does not apply (shape, dtype, policy, a block
    input of 2 GiB or more, an unaligned or non-contiguous operand)."""
    w, b = c3[0], c3[1]
    wp, bp, stride, pad = proj.f
    B, H, W, K = x.shape
    N, Kp = w.shape[0], proj.x.shape[3]
    w1, b1 = (c1_next[0], c1_next[1]) if c1_next is not None else (None, None)
    N2 = w1.shape[0] if w1 is not None else 0
    ts = [x, w, b, proj.x, wp, bp, w1, b1]
    if pad != 0 or tuple(wp.shape) != (N, 1, 1, Kp) or tuple(w.shape[1:]) != (1, 1, K) or proj.out_hw() != (H, W) \
            or proj.x.shape[0] != B or any(t.dtype != x.dtype for t in (w, proj.x, wp) + ((w1,) if N2 else ())) \
            or any(t is not None and (not t.is_contiguous() or t.data_ptr() % 16) for t in ts) \
            or proj.x.numel() * proj.x.element_size() >= 1 << 31 \
            or not conv1x1_proj_supported(B * H * W, K, N, Kp, stride, N2, x.dtype, policy):
        return None
    L.require_device(*[t for t in ts if t is not None])
    y = torch.empty(B, H, W, N, device=x.device, dtype=x.dtype)
    x1 = torch.empty(B, H, W, N2, device=x.device, dtype=x.dtype) if N2 else None
    L.check(L.lib().sat_conv1x1_proj(B, proj.x.shape[1], proj.x.shape[2], stride, K, N, Kp, N2, L.dtype_code(x.dtype),
                                     L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(proj.x), L.ptr(wp), L.ptr(bp), L.ptr(y),
                                     L.ptr(w1), L.ptr(b1), L.ptr(x1), L.policy_ptr(policy), L.stream_of(y)),
            "sat_conv1x1_proj")
    return y, x1


def conv2d_nhwc(x, w, bias, stride, pad, relu, residual=None, out=None, out_hw=None, policy=None):
    """x [N,H,W,C] ; w [Cout,KH,KW,C] (same dtype) ; bias f32 [Cout].  ``pad`` pads top/left;
    ``out_hw`` (default: symmetric padding) fixes the output size; ``policy``: optional per-call kernel
    selection (``sat_amd.Policy``).  ``residual`` may be a ProjectedResidual (a 1x1 / stride-1 conv + ReLU only)."""
    L.require_device(x, w)
    if isinstance(residual, ProjectedResidual):
        if relu and stride == 1 and pad == 0 and out is None and out_hw is None and w.shape[1] == w.shape[2] == 1:
            r = _proj_launch(x, (w, bias), residual, None, policy)
            if r is not None:
                return r[0]
        residual = residual.materialize(policy)
    N, H, W, C = x.shape
    Cout, KH, KW, Cw = w.shape
    assert Cw == C, (w.shape, x.shape)
    if out_hw is None:
        OH = (H + 2 * pad - KH) // stride + 1
        OW = (W + 2 * pad - KW) // stride + 1
    else:
        OH, OW = out_hw
    y = out if out is not None else torch.empty(N, OH, OW, Cout, device=x.device, dtype=x.dtype)
    g = L.SatConvGeom(N, H, W, C, KH, KW, stride, pad, OH, OW)
    if residual is not None:
        assert residual.shape == y.shape and residual.dtype == y.dtype
    L.check(L.lib().sat_conv2d_nhwc(ctypes.byref(g), Cout, L.dtype_code(x.dtype), L.ptr(x), L.ptr(w), L.ptr(bias),
                                    L.ptr(residual), int(relu), L.ptr(y), L.policy_ptr(policy), L.stream_of(y)),
            "sat_conv2d_nhwc")
    return y


def _stem_geom(x, w, stride, pad, out_hw):
    N, H, W, C = x.shape
    Cout, KH, KW, Cw = w.shape
    assert Cw == C, (w.shape, x.shape)
    if out_hw is None:
        out_hw = ((H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1)
    return L.SatConvGeom(N, H, W, C, KH, KW, stride, pad, out_hw[0], out_hw[1])


def conv_stem_pool_supported(x, w, stride, pad, relu, pool, out_hw=None, policy=None):
    """True when conv_stem_pool runs the conv (conv2d_nhwc's arguments) and the max pool ``pool`` = (k, stride, pad)
    as ONE launch under ``policy``."""
    g = _stem_geom(x, w, stride, pad, out_hw)
    return bool(L.lib().sat_conv_stem_pool_supported(ctypes.byref(g), w.shape[0], L.dtype_code(x.dtype), int(relu),
                                                     pool[0], pool[1], pool[2], L.policy_ptr(policy)))


def conv_stem_pool(x, w, bias, stride, pad, relu, pool, out_hw=None, policy=None):
    """maxpool2d_nhwc(conv2d_nhwc(x, w, bias, stride, pad, relu, out_hw=out_hw), *pool): ResNet152's stem.  One
    launch that never writes the conv's output when conv_stem_pool_supported (and the operands are contiguous and
    16-byte aligned), else the two launches; the same bits either way."""
    L.require_device(x, w, bias)
    ts = (x, w, bias)
    if all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0) for t in ts) and w.dtype == x.dtype \
            and conv_stem_pool_supported(x, w, stride, pad, relu, pool, out_hw, policy):
        g = _stem_geom(x, w, stride, pad, out_hw)
        k, ps, pp = pool
        y = torch.empty(g.N, (g.OH + 2 * pp - k) // ps + 1, (g.OW + 2 * pp - k) // ps + 1, w.shape[0], device=x.device,
                        dtype=x.dtype)
        L.check(L.lib().sat_conv_stem_pool(ctypes.byref(g), w.shape[0], L.dtype_code(x.dtype), L.ptr(x), L.ptr(w),
                                           L.ptr(bias), int(relu), k, ps, pp, L.ptr(y), L.policy_ptr(policy),
                                           L.stream_of(y)), "sat_conv_stem_pool")
        return y
    return maxpool2d_nhwc(conv2d_nhwc(x, w, bias, stride, pad, relu, out_hw=out_hw, policy=policy), *pool)


def mfma_frag_layout(w2d):
    """[N, K] bf16 -> the register-direct MFMA fragment layout sat_bottleneck_fused streams."""
    L.require_device(w2d)
    N, K = w2d.shape
    src = w2d.contiguous()
    dst = torch.empty_like(src)
    L.check(L.lib().sat_mfma_frag_layout(N, K, L.ptr(src), L.ptr(dst), L.stream_of(dst)), "sat_mfma_frag_layout")
    return dst


def bottleneck_fused_supported(H, W, Cin, Cmid, dtype):
    return bool(L.lib().sat_bottleneck_fused_supported(H, W, Cin, Cmid, L.dtype_code(dtype)))


def bottleneck_fused(x, f1, f2, f3, out=None, policy=None):
    """One identity-residual stride-1 bottleneck in one launch.  x NHWC [N,H,W,Cin]; f1/f2/f3 =
    (fragment-layout weight, fp32 bias) of the folded c1 / c2 / c3 (Encoder plan)."""
    L.require_device(x)
    N, H, W, C = x.shape
    Cmid = f1[1].shape[0]
    y = out if out is not None else torch.empty_like(x)
    L.check(L.lib().sat_bottleneck_fused(N, H, W, C, Cmid, L.dtype_code(x.dtype), L.ptr(x), L.ptr(f1[0]),
                                         L.ptr(f1[1]), L.ptr(f2[0]), L.ptr(f2[1]), L.ptr(f3[0]), L.ptr(f3[1]),
                                         L.ptr(y), L.policy_ptr(policy), L.stream_of(y)), "sat_bottleneck_fused")
    return y


def conv3x3_frag_supported(H, W, C, dtype):
    return bool(L.lib().sat_conv3x3_frag_supported(H, W, C, L.dtype_code(dtype)))


def conv3x3_frag(x, f, out=None, policy=None):
    """relu(conv3x3(x, pad 1) + b) with f = (fragment-layout weight, fp32 bias) of a folded [C][3][3][C]
    conv (a layer3 bottleneck's c2).  x NHWC [N,H,W,C]; bit-identical to conv2d_nhwc."""
    L.require_device(x)
    if not x.is_contiguous():
        raise ValueError("conv3x3_frag: x must be a contiguous NHWC tensor")
    N, H, W, C = x.shape
    y = out if out is not None else torch.empty_like(x)
    L.check(L.lib().sat_conv3x3_frag(N, H, W, C, L.dtype_code(x.dtype), L.ptr(x), L.ptr(f[0]), L.ptr(f[1]),
                                     L.ptr(y), L.policy_ptr(policy), L.stream_of(y)), "sat_conv3x3_frag")
    return y


def conv1x1_frag_supported(H, W, Cin, Cout, dtype):
    return bool(L.lib().sat_conv1x1_frag_supported(H, W, Cin, Cout, L.dtype_code(dtype)))


def conv1x1_frag(x, f, out=None, policy=None):
    """relu(x . W^T + b) with f = (fragment-layout weight, fp32 bias) of a folded [Cout][Cin] 1x1 conv (a
    layer3 bottleneck's c1).  x NHWC [N,H,W,Cin]; bit-identical to conv2d_nhwc."""
    L.require_device(x)
    if not x.is_contiguous():
        raise ValueError("conv1x1_frag: x must be a contiguous NHWC tensor")
    N, H, W, C = x.shape
    Cout = f[1].shape[0]
    y = out if out is not None else torch.empty(N, H, W, Cout, dtype=x.dtype, device=x.device)
    L.check(L.lib().sat_conv1x1_frag(N, H, W, C, Cout, L.dtype_code(x.dtype), L.ptr(x), L.ptr(f[0]), L.ptr(f[1]),
                                     L.ptr(y), L.policy_ptr(policy), L.stream_of(y)), "sat_conv1x1_frag")
    return y


def conv1x1_chain_supported(M, K, N, N2, dtype, policy=None):
    """True when conv1x1_chain runs (M pixels, K -> N channels, then N -> N2) as ONE launch under ``policy``."""
    return bool(L.lib().sat_conv1x1_chain_supported(M, K, N, N2, L.dtype_code(dtype), L.policy_ptr(policy)))


def conv1x1_chain(x, c3, residual, c1_next, policy=None):
    """A bottleneck's c3 and the next bottleneck's c1: y = relu(conv1x1(x, c3) + residual) and
    x1_next = relu(conv1x1(y, c1_next)), with c3 / c1_next = (w [Cout,1,1,Cin], bias f32, ...) as the Encoder plan
    folds them.  One launch when conv1x1_chain_supported (the c1 reads y's tile on chip), else the library issues
    the two launches; either way both outputs are bit-identical to two conv2d_nhwc calls.  ``residual`` may be a
    ProjectedResidual.  -> (y, x1_next)"""
    L.require_device(x, c3[0], c1_next[0])
    if isinstance(residual, ProjectedResidual):
        r = _proj_launch(x, c3, residual, c1_next, policy) if x.is_contiguous() else None
        if r is not None:
            return r
        residual = residual.materialize(policy)
    if not (x.is_contiguous() and residual.is_contiguous()):
        raise ValueError("conv1x1_chain: x and residual must be contiguous NHWC tensors")
    B, H, W, K = x.shape
    w, b, w1, b1 = c3[0], c3[1], c1_next[0], c1_next[1]
    N, N2 = w.shape[0], w1.shape[0]
    assert tuple(w.shape[1:]) == (1, 1, K) and tuple(w1.shape[1:]) == (1, 1, N), (w.shape, w1.shape, x.shape)
    assert w.dtype == x.dtype and w1.dtype == x.dtype
    y = torch.empty(B, H, W, N, device=x.device, dtype=x.dtype)
    assert residual.shape == y.shape and residual.dtype == y.dtype
    x1 = torch.empty(B, H, W, N2, device=x.device, dtype=x.dtype)
    L.check(L.lib().sat_conv1x1_chain(B * H * W, K, N, N2, L.dtype_code(x.dtype), L.ptr(x), L.ptr(w), L.ptr(b),
                                      L.ptr(residual), L.ptr(y), L.ptr(w1), L.ptr(b1), L.ptr(x1),
                                      L.policy_ptr(policy), L.stream_of(y)), "sat_conv1x1_chain")
    return y, x1


def conv3x3_wgrad_workspace_bytes(x_shape, cout, dtype, policy=None):
    """Bytes of the split-K workspace conv3x3_wgrad uses for an NHWC input of ``x_shape`` and ``cout`` output channels
    under ``policy``; 0 for a shape the kernel refuses."""
    N, H, W, C = x_shape
    return int(L.lib().sat_conv3x3_wgrad_workspace_bytes(N, H, W, C, cout, L.dtype_code(dtype), L.policy_ptr(policy)))


def conv3x3_wgrad(x, dz, out=None, accumulate=False, policy=None, workspace=True):
    """Weight gradient of a 3x3 / stride-1 / pad-1 conv: x NHWC [N,H,W,Cin], dz NHWC [N,H,W,Cout] (bf16) ->
    dw fp32 [Cout,3,3,Cin] (the folded weight's order), ``out`` overwritten or, with ``accumulate``, added to.
    Cin and Cout multiples of 128; anything else raises (no second path).  ``workspace``: True = a split-K workspace
    allocated for this call, a uint8 device tensor of at least conv3x3_wgrad_workspace_bytes, or None (unsplit)."""
    L.require_device(x, dz, out)
    if x.dtype != dz.dtype or x.shape[:3] != dz.shape[:3]:
        raise ValueError(f"conv3x3_wgrad: x{tuple(x.shape)} {x.dtype} and dz{tuple(dz.shape)} {dz.dtype} do not match")
    if not (x.is_contiguous() and dz.is_contiguous()):
        raise ValueError("conv3x3_wgrad: x and dz must be contiguous NHWC tensors")
    N, H, W, Cin = x.shape
    Cout = dz.shape[3]
    if out is None:
        if accumulate:
            raise ValueError("conv3x3_wgrad: accumulate needs the buffer to add to")
        out = torch.empty(Cout, 3, 3, Cin, device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (Cout, 3, 3, Cin) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("conv3x3_wgrad: out must be a contiguous fp32 [Cout,3,3,Cin] tensor")
    if workspace is True:
        workspace = torch.empty(conv3x3_wgrad_workspace_bytes(x.shape, Cout, x.dtype, policy), dtype=torch.uint8,
                                device=x.device)
    ws_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    L.check(L.lib().sat_conv3x3_wgrad(N, H, W, Cin, Cout, L.dtype_code(x.dtype), L.ptr(x), L.ptr(dz), L.ptr(out),
                                      int(accumulate), L.ptr(workspace) if ws_bytes else None, ws_bytes,
                                      L.policy_ptr(policy), L.stream_of(out)), "sat_conv3x3_wgrad")
    return out


def maxpool2d_nhwc(x, k, stride, pad=0):
    L.require_device(x)
    N, H, W, C = x.shape
    OH = (H + 2 * pad - k) // stride + 1
    OW = (W + 2 * pad - k) // stride + 1
    y = torch.empty(N, OH, OW, C, device=x.device, dtype=x.dtype)
    L.check(L.lib().sat_maxpool2d_nhwc(N, H, W, C, k, stride, pad, L.dtype_code(x.dtype), L.ptr(x), L.ptr(y), OH, OW,
                                       L.stream_of(y)), "sat_maxpool2d_nhwc")
    return y


def _rows_args(what, table, idx, batch, n_bad):
    """Checks shared by rows_gather / rows_scatter: ``table`` [n_rows, ...] and ``batch`` [n, ...] contiguous with equal
    row shapes and dtype, ``idx`` int64 [n], ``n_bad`` one int32 -> (n_rows, row_elems)."""
    L.require_device(table, idx, batch, n_bad)
    if table.dim() < 1 or table.shape[0] == 0 or not table.is_contiguous():
        raise ValueError(f"{what}: table must be a contiguous [n_rows, ...] tensor with n_rows > 0")
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError(f"{what}: idx must be a contiguous int64 vector")
    if batch.dtype != table.dtype or tuple(batch.shape) != (idx.shape[0],) + tuple(table.shape[1:]) \
            or not batch.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {table.dtype} batch of shape "
                         f"{(idx.shape[0],) + tuple(table.shape[1:])}, got {batch.dtype} {tuple(batch.shape)}")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1):
        raise ValueError(f"{what}: n_bad must be one int32")
    row_elems = table.numel() // table.shape[0]
    if row_elems == 0:
        raise ValueError(f"{what}: empty rows")
    return table.shape[0], row_elems


def rows_gather(table, idx, out=None, n_bad=None):
    """out[i] = table[idx[i]] (sat_rows_gather): ``table`` [n_rows, ...] bf16 / fp32, ``idx`` int64 [n] on the device.
    A row whose index lies outside the table comes out zero and adds 1 to ``n_bad`` (one int32 on the device, zeroed
    by the caller) when that is given."""
    if out is None:
        L.require_device(table, idx)
        out = torch.empty((idx.shape[0],) + tuple(table.shape[1:]), device=table.device, dtype=table.dtype)
    n_rows, row_elems = _rows_args("rows_gather", table, idx, out, n_bad)
    if idx.shape[0] == 0:   # an empty tensor has no pointer to hand over
        return out
    L.check(L.lib().sat_rows_gather(L.ptr(table), n_rows, row_elems, L.dtype_code(table.dtype), L.ptr(idx),
                                    idx.shape[0], L.ptr(out), L.ptr(n_bad), L.stream_of(out)), "sat_rows_gather")
    return out


def rows_scatter(src, idx, table, n_bad=None):
    """table[idx[i]] = src[i] (sat_rows_scatter), the indices distinct.  A row whose index lies outside the table is
    skipped and adds 1 to ``n_bad`` when that is given."""
    n_rows, row_elems = _rows_args("rows_scatter", table, idx, src, n_bad)
    if idx.shape[0] == 0:
        return table
    L.check(L.lib().sat_rows_scatter(L.ptr(src), idx.shape[0], row_elems, L.dtype_code(table.dtype), L.ptr(idx),
                                     L.ptr(table), n_rows, L.ptr(n_bad), L.stream_of(table)), "sat_rows_scatter")
    return table


CIDER_MAX_WORDS = 64        # words of a hypothesis row / a reference the device scorer takes
CIDER_ID_LIMIT = 1 << 20    # token ids are below this (the sampling entries' limit)


def _cider_table_args(what, table):
    L.require_device(table)
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 2 \
            or not table.is_contiguous():
        raise ValueError(f"{what}: table must be a contiguous int32 [slots, 4] tensor with slots >= 2")
    return table.shape[0]


def _cider_keys_args(what, table, keys, other, other_dtype):
    L.require_device(keys, other)
    if keys.dtype != torch.int32 or keys.dim() != 2 or keys.shape[1] != 3 or not keys.is_contiguous() \
            or keys.device != table.device:
        raise ValueError(f"{what}: keys must be a contiguous int32 [n, 3] tensor on the table's device")
    if other.dtype != other_dtype or tuple(other.shape) != (keys.shape[0],) or not other.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous {other_dtype} vector of {keys.shape[0]} elements")


def cider_table_insert(table, keys, values, n_bad=None):
    """Store the packed n-gram ``keys`` (int32 [n, 3], the bit pattern of sat_hip.h's key words; unique) with their fp32
    ``values`` in ``table`` (int32 [slots, 4], zeroed before the first insert).  A key that finds no slot adds 1 to
    ``n_bad`` (one int32 on the device)."""
    slots = _cider_table_args("cider_table_insert", table)
    _cider_keys_args("cider_table_insert", table, keys, values, torch.float32)
    L.require_device(n_bad)
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1):
        raise ValueError("cider_table_insert: n_bad must be one int32")
    if keys.shape[0]:
        L.check(L.lib().sat_cider_table_insert(L.ptr(table), slots, L.ptr(keys), L.ptr(values), keys.shape[0],
                                               L.ptr(n_bad), L.stream_of(table)), "sat_cider_table_insert")
    return table


def cider_lookup(table, log_n, keys, out=None):
    """out[i] = the value stored under keys[i], ``log_n`` for a key that was never inserted (sat_cider_lookup)."""
    slots = _cider_table_args("cider_lookup", table)
    if out is None:
        L.require_device(keys)
        out = torch.empty(keys.shape[0], device=keys.device, dtype=torch.float32)
    _cider_keys_args("cider_lookup", table, keys, out, torch.float32)
    if keys.shape[0]:
        L.check(L.lib().sat_cider_lookup(L.ptr(table), slots, float(log_n), L.ptr(keys), keys.shape[0], L.ptr(out),
                                         L.stream_of(out)), "sat_cider_lookup")
    return out


def _cider_refs_args(what, table, ref_words, ref_len, ref_norm):
    L.require_device(ref_words, ref_len, ref_norm)
    n_refs = ref_len.shape[0] if ref_len.dim() == 1 else -1
    if ref_words.dtype != torch.int32 or ref_words.dim() != 2 or not ref_words.is_contiguous() \
            or ref_words.shape[0] < max(1, n_refs) or not 1 <= ref_words.shape[1] <= CIDER_MAX_WORDS:
        raise ValueError(f"{what}: ref_words must be a contiguous int32 [n_refs, stride <= {CIDER_MAX_WORDS}] tensor")
    if ref_len.dtype != torch.int32 or n_refs < 0 or not ref_len.is_contiguous():
        raise ValueError(f"{what}: ref_len must be a contiguous int32 vector")
    if ref_norm.dtype != torch.float32 or ref_norm.dim() != 2 or ref_norm.shape[1] != 4 \
            or ref_norm.shape[0] < max(1, n_refs) or not ref_norm.is_contiguous():
        raise ValueError(f"{what}: ref_norm must be a contiguous float32 [n_refs, 4] tensor")
    if not (ref_words.device == ref_len.device == ref_norm.device == table.device):
        raise ValueError(f"{what}: the corpus tensors must live on one device")
    return n_refs, ref_words.shape[1]


def cider_ref_norms(table, log_n, ref_words, ref_len, ref_norm):
    """ref_norm[r, n - 1] = the norm of reference r's tf-idf vector of n-grams (sat_cider_ref_norms)."""
    slots = _cider_table_args("cider_ref_norms", table)
    n_refs, stride = _cider_refs_args("cider_ref_norms", table, ref_words, ref_len, ref_norm)
    if n_refs:
        L.check(L.lib().sat_cider_ref_norms(L.ptr(table), slots, float(log_n), L.ptr(ref_words), L.ptr(ref_len),
                                            n_refs, stride, L.ptr(ref_norm), L.stream_of(ref_norm)),
                "sat_cider_ref_norms")
    return ref_norm


def cider_score(table, log_n, ref_words, ref_len, ref_norm, img_ref_begin, tokens, image, ids, out=None, n_bad=None):
    """CIDEr-D of every row of ``tokens`` (int32 [n, T1 <= 64], device) against the references of ``image`` (int64
    [n], device) -> float32 [n] (sat_cider_score); ``ids`` = (start, end, pad).  No host read: capturable."""
    slots = _cider_table_args("cider_score", table)
    n_refs, stride = _cider_refs_args("cider_score", table, ref_words, ref_len, ref_norm)
    L.require_device(img_ref_begin, tokens, image, n_bad)
    if img_ref_begin.dtype != torch.int32 or img_ref_begin.dim() != 1 or img_ref_begin.shape[0] < 1 \
            or not img_ref_begin.is_contiguous() or img_ref_begin.device != table.device:
        raise ValueError("cider_score: img_ref_begin must be a contiguous int32 [n_images + 1] vector")
    if tokens.dtype != torch.int32 or tokens.dim() != 2 or not tokens.is_contiguous() \
            or not 1 <= tokens.shape[1] <= CIDER_MAX_WORDS or tokens.device != table.device:
        raise ValueError(f"cider_score: tokens must be a contiguous int32 [n, T1] tensor on the corpus' device with "
                         f"1 <= T1 <= {CIDER_MAX_WORDS}, got {tokens.dtype} {tuple(tokens.shape)}")
    if image.dtype != torch.int64 or tuple(image.shape) != (tokens.shape[0],) or not image.is_contiguous() \
            or image.device != table.device:
        raise ValueError(f"cider_score: image must be a contiguous int64 vector of {tokens.shape[0]} elements on the "
                         f"corpus' device, got {image.dtype} {tuple(image.shape)}")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1):
        raise ValueError("cider_score: n_bad must be one int32")
    if out is None:
        out = torch.empty(tokens.shape[0], device=tokens.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (tokens.shape[0],) or not out.is_contiguous() \
            or out.device != table.device:
        raise ValueError("cider_score: out must be a contiguous float32 [n] tensor on the corpus' device")
    if tokens.shape[0]:
        start_id, end_id, pad_id = (int(i) for i in ids)
        L.check(L.lib().sat_cider_score(L.ptr(table), slots, float(log_n), L.ptr(ref_words), L.ptr(ref_len),
                                        L.ptr(ref_norm), n_refs, stride, L.ptr(img_ref_begin),
                                        img_ref_begin.shape[0] - 1, L.ptr(tokens), L.ptr(image), tokens.shape[0],
                                        tokens.shape[1], start_id, end_id, pad_id, L.ptr(out), L.ptr(n_bad),
                                        L.stream_of(out)), "sat_cider_score")
    return out


def adam_step_(param, grad, exp_avg, exp_avg_sq, param_lp, beta1, beta2, eps, step_size, bc2_sqrt):
    L.check(L.lib().sat_adam_step(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), L.ptr(param_lp),
                                  param.numel(), beta1, beta2, eps, step_size, bc2_sqrt, L.stream_of(param)),
            "sat_adam_step")


GRAD_SUMSQ_SWEEP = 4096      # fp32 elements one workgroup of sat_grad_sumsq reads per loop trip (csrc/elementwise.hip)
GRAD_SUMSQ_MAX_PARTIALS = 1024


def grad_sumsq_partials(n):
    """Workgroups (= partials) ``sat_grad_sumsq`` gets for a range of ``n`` elements: one per sweep, at most
    ``GRAD_SUMSQ_MAX_PARTIALS`` (4 workgroups per CU, 64 KiB of loads in flight on each)."""
    return max(1, min(GRAD_SUMSQ_MAX_PARTIALS, -(-int(n) // GRAD_SUMSQ_SWEEP)))


def grad_sumsq(grad, partials):
    """partials[i] = the fp64 sum of squares of workgroup i's share of ``grad`` (fp32, contiguous); every element of
    ``partials`` (float64 vector) is written."""
    L.require_device(grad, partials)
    if grad.dtype != torch.float32 or not grad.is_contiguous():
        raise TypeError("grad_sumsq: grad must be a contiguous float32 tensor")
    if partials.dtype != torch.float64 or partials.dim() != 1 or not partials.is_contiguous() \
            or partials.numel() < 1 or partials.device != grad.device:
        raise TypeError("grad_sumsq: partials must be a non-empty contiguous float64 vector on grad's device")
    L.check(L.lib().sat_grad_sumsq(L.ptr(grad), grad.numel(), L.ptr(partials), partials.numel(),
                                   L.stream_of(grad)), "sat_grad_sumsq")
    return partials


def grad_clip_finalize(partials, max_norm, state):
    """state[0:3] = (norm, scale, non-finite flag) from the fp64 ``partials`` of every range; state[3] += the flag."""
    L.require_device(partials, state)
    if partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() < 1:
        raise TypeError("grad_clip_finalize: partials must be a non-empty contiguous float64 vector")
    if state.dtype != torch.float32 or not state.is_contiguous() or state.numel() != 4 \
            or state.device != partials.device:
        raise TypeError("grad_clip_finalize: state must be 4 contiguous float32 on the partials' device")
    L.check(L.lib().sat_grad_clip_finalize(L.ptr(partials), partials.numel(), float(max_norm), L.ptr(state),
                                           L.stream_of(state)), "sat_grad_clip_finalize")
    return state


def adam_step_scaled_(param, grad, exp_avg, exp_avg_sq, param_lp, beta1, beta2, eps, step_size, bc2_sqrt, state):
    """``adam_step_`` on ``grad * state[1]``; a no-op when ``state[2] != 0`` (``grad_clip_finalize``'s state)."""
    L.require_device(param, grad, exp_avg, exp_avg_sq, param_lp, state)
    L.check(L.lib().sat_adam_step_scaled(L.ptr(param), L.ptr(grad), L.ptr(exp_avg), L.ptr(exp_avg_sq),
                                         L.ptr(param_lp), param.numel(), beta1, beta2, eps, step_size, bc2_sqrt,
                                         L.ptr(state), L.stream_of(param)), "sat_adam_step_scaled")

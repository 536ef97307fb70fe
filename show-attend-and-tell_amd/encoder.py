"""Encoder module (reference: encoder.py:5-40) on MFMA implicit-GEMM convolutions.

``Encoder(network)`` keeps the reference attributes (``network``, ``net``,
``dim``) and the torchvision 0.16 parameter layout of ``self.net``
(``vgg19().features[:-1]`` -> keys ``net.<i>.weight``; ``resnet152`` children
``[:-2]`` -> ``net.0`` conv1, ``net.1`` bn1, ``net.4-7`` layer1-4 Bottlenecks), so
torchvision-derived state_dicts load unchanged.  ``forward(x[B,3,H,W]) ->
[B, L, D]`` runs the trunk as a compiled plan of HIP kernels on NHWC
activations:

  * every Conv2d (+ eval-mode BatchNorm folded into weight/bias, + ReLU, + the
    residual add of a Bottleneck) is ONE implicit-GEMM MFMA launch
    (sat_conv2d_nhwc): M = B*OH*OW, N = Cout, K = KH*KW*Cin;
  * in ResNet152's layer1 a block's c3 launch also computes the next block's c1 from its
    output tile while that is still on chip (ops.conv1x1_chain; ``Encoder.chain_c1``);
  * at the trunk's entry no tensor is written only to be read straight back: ResNet152's stem conv and its max
    pool are one launch (ops.conv_stem_pool; ``Encoder.stem_pool``), and the projection shortcut of layer1's and
    layer2's first block is computed inside that block's c3 launch (ops.ProjectedResidual; ``proj_l1``, ``proj_l2``);
  * every other MaxPool2d is a streaming NHWC kernel;
  * the image is converted once to NHWC with channels zero-padded 3 -> 8 so the
    first conv loads 16-byte vectors (VGG19); for ResNet152 it is converted to a
    2x2 space-to-depth layout instead ([H/2, W/2, 16], 12 real channels) and the
    7x7 / stride-2 / pad-3 stem runs as the equivalent 4x4 / stride-1 conv with
    re-laid-out weights (K = 256 instead of 7*7*8 = 392, half the input bytes);
  * the final NHWC tensor already IS ``permute(0,2,3,1).view(B,-1,C)``
    (encoder.py:37-39): no transpose.

By default the trunk is frozen (``requires_grad=False``) and forward-only for
every network: the reference freezes only VGG19 (encoder.py:29-31) and lets
ResNet152 accumulate encoder gradients the optimiser never reads (train.py:71);
skipping that dead backward leaves every trained value identical.
``Encoder(..., fine_tune=n)`` / ``Encoder.fine_tune(n)`` makes the last ``n``
units trainable (ResNet152: layer4's identity bottlenecks, n <= 2; VGG19: the
block-5 convolutions, n <= 4): with grad enabled the forward runs plan steps
``tail_start()`` .. end through ``_TailFn``, whose backward consumes the decoder's
``dL/d(img_features)`` and leaves the tail's gradients in views of
``Encoder.tail_grad_flat``.  BatchNorm stays in eval mode.
Pretrained ImageNet weights are a download in the reference; here weights are
randomly initialised with torchvision's scheme unless a state_dict is loaded.
DenseNet161 (argparse choice, no BASELINE config) is out of scope.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .data import PackedImages

VGG19_CFG = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]
IN_PAD = 8  # input channels padded 3 -> 8 (16-B bf16 vectors in the im2col loader)
S2D_C = 16  # space-to-depth stem input channels (2*2*3 real, zero-padded)


def stem_weight_s2d(w):
    """[Cout, KH=7, KW=7, Cin<=4] (NHWC-ordered, folded) stride-2 / pad-3 stem weights -> the
    [Cout, 4, 4, 16] weights of the same conv over the space-to-depth input: input row
    ih = 2*oh - 3 + kh = 2*(oh - 2 + th) + sy with kh + 1 = 2*th + sy, so tap (th, tw) and
    sub-pixel (sy, sx) of channel c land in s2d channel (sy*2 + sx)*Cin + c; the (kh + 1 = 0)
    row / column of the 8x8 footprint carries zero weight."""
    cout, kh_n, kw_n, cin = w.shape
    assert kh_n == 7 and kw_n == 7 and 4 * cin <= S2D_C
    out = torch.zeros(cout, 4, 4, S2D_C, dtype=w.dtype, device=w.device)
    for kh in range(7):
        th, sy = divmod(kh + 1, 2)
        for kw in range(7):
            tw, sx = divmod(kw + 1, 2)
            c0 = (sy * 2 + sx) * cin
            out[:, th, tw, c0:c0 + cin] = w[:, kh, kw, :]
    return out


class Bottleneck(nn.Module):
    """torchvision Bottleneck (expansion 4, stride on the 3x3: ResNet v1.5)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _vgg19_features():
    layers, cin = [], 3
    for v in VGG19_CFG:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return layers[:-1]   # encoder.py:24-27 drops the last MaxPool


def _resnet152_trunk():
    layers = [nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
              nn.MaxPool2d(3, 2, 1)]
    inplanes = 64
    for li, (n, planes) in enumerate(zip([3, 8, 36, 3], [64, 128, 256, 512])):
        stride = 1 if li == 0 else 2
        blocks = []
        for bi in range(n):
            s = stride if bi == 0 else 1
            ds = None
            if bi == 0 and (s != 1 or inplanes != planes * 4):
                ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=s, bias=False), nn.BatchNorm2d(planes * 4))
            blocks.append(Bottleneck(inplanes, planes, s, ds))
            inplanes = planes * 4
        layers.append(nn.Sequential(*blocks))
    return layers


def _init_like_torchvision(module):
    """torchvision's init (kaiming-normal fan_out convs, BN gamma=1 beta=0), except that the
    last BN of every Bottleneck starts at gamma=0.2: with plain gamma=1 the 50 residual
    blocks double the activation variance per block (output std ~1e7 at random init),
    whereas a pretrained trunk -- which this random init stands in for -- emits O(1)
    features.  (torchvision's own zero_init_residual option uses gamma=0, which would feed
    the conv3 MFMAs all-zero weights and flatter their timing.)"""
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    for m in module.modules():
        if isinstance(m, Bottleneck):
            nn.init.constant_(m.bn3.weight, 0.2)


FINE_TUNE_LIMIT = {"resnet152": 2, "vgg19": 4}
VGG19_TAIL_CONVS = (28, 30, 32, 34)   # block 5: net.<i>, in forward order


class _TailFn(torch.autograd.Function):
    """The trainable tail of the trunk (plan steps k .. end) with a backward: the forward is the plan's own c1 / c2 /
    c3 (or conv) launches, keeping each unit's activations; the backward is one C-ABI call per unit
    (sat_bottleneck_backward / sat_conv3x3_relu_backward), last unit first, into views of ``Encoder.tail_grad_flat``."""

    @staticmethod
    def forward(ctx, act, enc, first, *params):
        plan = enc._plan
        k = enc.tail_start()
        y, saved = act, []
        for step in plan[k + first:]:
            y, sv = enc._tail_unit_forward(y, step)
            saved.append(sv)
        ctx.enc, ctx.first, ctx.saved = enc, first, saved
        ctx.trains = [enc._tail_state[first + i] for i in range(len(saved))]
        B, H, W, C = y.shape
        return y.view(B, H * W, C)

    @staticmethod
    def backward(ctx, d_feats):
        enc, saved = ctx.enc, ctx.saved
        out = saved[-1][-1]
        if d_feats.dtype != out.dtype:
            raise TypeError("sat_amd.Encoder.backward: grad dtype must match the features")
        dy = d_feats.contiguous().view(out.shape)
        accumulate = enc._attach_tail_grads()
        lib = L.lib()
        dt = L.dtype_code(out.dtype)
        pol = L.policy_ptr(enc.policy)
        sizes = []
        for sv in saved:
            N, H, W, Cin = sv[0].shape
            fn = lib.sat_bottleneck_backward_workspace_bytes if len(sv) == 4 else \
                lib.sat_conv3x3_relu_backward_workspace_bytes
            sizes.append(fn(N, H, W, Cin, sv[1].shape[3], dt, pol))
            if sizes[-1] == 0:
                raise RuntimeError(f"sat_amd.Encoder.backward: unsupported tail shape {tuple(sv[0].shape)}")
        ws = torch.empty(max(sizes), device=out.device, dtype=torch.uint8)
        stream = L.stream_of(out)
        for i in reversed(range(len(saved))):
            sv, tr = saved[i], ctx.trains[i]
            x = sv[0]
            N, H, W, Cin = x.shape
            dx = torch.empty_like(x) if i > 0 or ctx.needs_input_grad[0] else None
            cts = [t.conv_train(enc.tail_grad_flat) for t in tr]
            if len(sv) == 4:
                L.check(lib.sat_bottleneck_backward(N, H, W, Cin, sv[1].shape[3], dt, L.ptr(x), L.ptr(sv[1]),
                                                    L.ptr(sv[2]), L.ptr(sv[3]), ctypes.byref(cts[0]),
                                                    ctypes.byref(cts[1]), ctypes.byref(cts[2]), L.ptr(dy), L.ptr(dx),
                                                    int(accumulate), L.ptr(ws), ws.numel(), pol, stream),
                        "sat_bottleneck_backward")
            else:
                L.check(lib.sat_conv3x3_relu_backward(N, H, W, Cin, sv[1].shape[3], dt, L.ptr(x), L.ptr(sv[1]),
                                                      ctypes.byref(cts[0]), L.ptr(dy), L.ptr(dx), int(accumulate),
                                                      L.ptr(ws), ws.numel(), pol, stream),
                        "sat_conv3x3_relu_backward")
            dy = dx
        ctx.saved = None
        return (dy if ctx.needs_input_grad[0] else None, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


class _TailConv:
    """One trainable conv of the tail: its modules, its folded buffers (written in place by sat_conv_fold at every
    refresh) and the offsets of its gradients in ``Encoder.tail_grad_flat``."""

    def __init__(self, conv, bn, device, dtype, frag):
        self.conv, self.bn = conv, bn
        co, ci, kh, kw = conv.weight.shape
        self.w_fold = torch.empty(co, kh, kw, ci, device=device, dtype=dtype)
        self.b_fold = torch.empty(co, device=device, dtype=torch.float32)
        self.w_igrad = torch.empty(ci, kh, kw, co, device=device, dtype=dtype) if kh == 3 else None
        self.frag = torch.empty(co, kh * kw * ci, device=device, dtype=dtype) if frag else None
        self.offsets = {}   # parameter -> element offset in tail_grad_flat

    def params(self):
        ps = [self.conv.weight] + ([self.conv.bias] if self.conv.bias is not None else [])
        return ps + ([self.bn.weight, self.bn.bias] if self.bn is not None else [])

    def fold(self, stream):
        c, bn = self.conv, self.bn
        co, ci, kh, kw = c.weight.shape
        lib = L.lib()
        L.check(lib.sat_conv_fold(co, ci, kh, kw, L.dtype_code(self.w_fold.dtype), L.ptr(c.weight), L.ptr(c.bias),
                                  L.ptr(bn.weight if bn else None), L.ptr(bn.bias if bn else None),
                                  L.ptr(bn.running_mean if bn else None), L.ptr(bn.running_var if bn else None),
                                  bn.eps if bn else 0.0, L.ptr(self.w_fold), L.ptr(self.b_fold), L.ptr(self.w_igrad),
                                  stream), "sat_conv_fold")
        if self.frag is not None:   # the forward reads this conv's weight in the fragment layout
            L.check(lib.sat_mfma_frag_layout(co, kh * kw * ci, L.ptr(self.w_fold), L.ptr(self.frag), stream),
                    "sat_mfma_frag_layout")

    def folded(self):
        return (self.w_fold, self.b_fold, self.conv.stride[0], self.conv.padding[0])

    def conv_train(self, flat):
        c, bn = self.conv, self.bn
        base = flat.data_ptr()

        def g(p):
            return None if p is None else ctypes.c_void_p(base + 4 * self.offsets[p])
        t = L.SatConvTrain()
        t.weight, t.bias = c.weight.data_ptr(), L.ptr(c.bias)
        if bn is not None:
            t.bn_weight, t.bn_mean, t.bn_var, t.eps = (bn.weight.data_ptr(), bn.running_mean.data_ptr(),
                                                       bn.running_var.data_ptr(), bn.eps)
            t.bn_weight_grad, t.bn_bias_grad = g(bn.weight), g(bn.bias)
        t.w_fold, t.w_igrad = self.w_fold.data_ptr(), L.ptr(self.w_igrad)
        t.weight_grad, t.bias_grad = g(c.weight), g(c.bias)
        return t


class Encoder(nn.Module):
    def __init__(self, network="vgg19", dtype=torch.float32, fine_tune=0):
        super().__init__()
        self.network = network
        if network == "resnet152":
            self.net = nn.Sequential(*_resnet152_trunk())
            self.dim = 2048
        elif network == "densenet161":
            raise NotImplementedError("densenet161 is out of scope for the MI355X path (no BASELINE config)")
        else:
            self.net = nn.Sequential(*_vgg19_features())
            self.dim = 512
        _init_like_torchvision(self.net)
        for p in self.net.parameters():   # frozen trunk (encoder.py:29-31; see module docstring)
            p.requires_grad = False
        self.compute_dtype = dtype
        self._plan = None
        self._plan_key = None
        self.timing = None   # bench hook: list collecting (start, end) HIP events around every conv launch
        self.timing_args = None   # bench hook: list collecting every conv launch's arguments
        # (a fused bottleneck launch is recorded as ("fused", x, frags))
        # bench hook: callable() -> the SatPolicy of the next conv launch (bench.py gives every launch its own
        # in-kernel timestamp slots, SatPolicy.stamps); None = self.policy for every launch
        self.launch_policy = None
        # identity-residual bottlenecks the fused kernel supports run as ONE launch
        # (sat_bottleneck_fused, csrc/convblock.hip); False = three conv launches (A/B, tests);
        # an int n fuses every n-th eligible block only (the unfused ones leave CUs to a decoder
        # running beside the encoder: bench.py --fuse-every)
        self.fuse_blocks = True
        # layer2's identity bottlenecks (28 x 28, 512 -> 128) as ONE launch each (the band form of
        # sat_bottleneck_fused); independent of fuse_blocks, which governs the 14 x 14 layer3 blocks.  Off: at
        # B = 128 the fused band kernel is no faster than the three launches (112 vs 106 us; B = 64: 51 vs 60)
        # and its 159 KB of LDS per CU slow the overlapped train step (profiles/r3_s22)
        self.fuse_layer2 = False
        # the c2 of an identity block left unfused runs on the half-image conv kernel
        # (sat_conv3x3_frag: input rows staged once in LDS, fragment-layout weights); False = the
        # tile kernel (A/B, tests)
        self.c2_frag = True
        # ... at these spatial sizes (layer4 7, layer3 14, layer2 28; VGG19 block 5 14, block 2 112);
        # A/B: bench.py --c2-frag-sizes
        self.c2_frag_sizes = (7, 14, 28, 56, 112)
        # ... its c1 on the half-image 1x1 kernel (sat_conv1x1_frag: input slabs by LDS-DMA, weights
        # register-direct)
        self.c1_frag = True
        # c3 input widths (64: layer1, 128: layer2) whose c3 + residual launch also computes the NEXT unfused block's
        # c1 from its output tile while that is still on chip (ops.conv1x1_chain, csrc/convstream.hip): the next
        # block then launches no c1 and the c3's output is not read back for it.  set() = every c1 its own launch
        # (A/B, tests).  Layer2 (128) is off: its chained kernel is faster than the two launches on its own but
        # slows the overlapped train step (5.95 vs 5.90 ms)
        self.chain_c1 = {64}
        # ResNet152's stem conv and the max pool behind it as ONE launch that never writes the 112 x 112 tensor
        # (ops.conv_stem_pool, csrc/conv3x3ws.hip), when both are in the forward's slice.  False = conv, then pool
        self.stem_pool = True
        # the projection shortcut of layer1's / layer2's first block computed inside its c3 launch from the block
        # input's tile (ops.ProjectedResidual, csrc/convstream.hip): no downsample launch, and its output is neither
        # written nor read back.  False = the downsample conv its own launch (A/B, tests)
        self.proj_l1 = True
        self.proj_l2 = True
        # per-call kernel selection for the conv launches (sat_amd.Policy / SatPolicy; None = the library's
        # defaults): A/B measurements and tests only
        self.policy = None
        # the trainable tail (fine_tune): units, their folded buffers per (device, dtype), the flat gradient buffer
        self._fine_tune = 0
        self._tail_state = None
        self._tail_state_key = None
        self._tail_key_done = None
        self.tail_grad_flat = None
        if fine_tune:
            self.fine_tune(fine_tune)

    # ---- the trainable tail ---------------------------------------------------
    def _tail_units(self, n=None):
        """The last ``n`` trainable units in forward order, each a list of (conv, bn or None)."""
        n = self._fine_tune if n is None else n
        if n == 0:
            return []
        if self.network == "resnet152":   # the identity bottlenecks of layer4, counted from the end
            blocks = list(self.net[7])[-n:]
            return [[(b.conv1, b.bn1), (b.conv2, b.bn2), (b.conv3, b.bn3)] for b in blocks]
        return [[(self.net[i], None)] for i in VGG19_TAIL_CONVS[-n:]]

    def fine_tune(self, n):
        """Make the last ``n`` units of the trunk trainable (0 = the frozen encoder): ResNet152's layer4 identity
        bottlenecks from the end (net.7.2, net.7.1), VGG19's block-5 convolutions (net.34, .32, .30, .28).  Their conv
        weights (and biases) and BatchNorm affine parameters get ``requires_grad``; BatchNorm stays in eval mode and
        its running statistics are never touched."""
        limit = FINE_TUNE_LIMIT[self.network]
        if not 0 <= int(n) <= limit:
            raise ValueError(f"Encoder.fine_tune: {self.network} has at most {limit} trainable units, got {n}")
        self._fine_tune = int(n)
        for p in self.net.parameters():
            p.requires_grad = False
        for unit in self._tail_units():
            for conv, bn in unit:
                for p in [conv.weight, conv.bias] + ([bn.weight, bn.bias] if bn is not None else []):
                    if p is not None:
                        p.requires_grad = True
        self._plan = self._plan_key = self._tail_state = self._tail_state_key = self._tail_key_done = None
        self.tail_grad_flat = None
        return self

    def tail_parameters(self):
        """The trainable tail's parameters in ``tail_grad_flat`` order."""
        return [p for unit in self._tail_units() for conv, bn in unit
                for p in [conv.weight, conv.bias] + ([bn.weight, bn.bias] if bn is not None else []) if p is not None]

    def _plan_len(self):
        return 52 if self.network == "resnet152" else 20   # stem, pool, 50 blocks | 16 convs, 4 pools

    def tail_start(self):
        """The plan index where the trainable tail begins (the plan's length when nothing is trainable)."""
        return self._plan_len() - self._fine_tune

    def _tail_tensors(self):
        """Parameters and buffers of the tail's units: their versions make the tail part of the state key."""
        ts = []
        for unit in self._tail_units():
            for conv, bn in unit:
                ts += list(conv.parameters()) + (list(bn.parameters()) + list(bn.buffers()) if bn is not None else [])
        return ts

    def _tail_key(self):
        return tuple(t._version for t in self._tail_tensors())

    def _refold_tail(self, device, dtype):
        """Fold the tail's convs with sat_conv_fold into their own buffers and point the tail's plan entries at them;
        the prefix's entries are not touched."""
        skey = (device, dtype)
        if self._tail_state is None or self._tail_state_key != skey:
            state = []
            for unit in self._tail_units():
                convs = []
                for conv, bn in unit:
                    if conv.weight.dtype != torch.float32 or not conv.weight.is_contiguous():
                        raise TypeError("Encoder.fine_tune: the tail's parameters must be contiguous float32")
                    cmid = conv.out_channels
                    hw = 7 if self.network == "resnet152" else 14
                    frag = conv.kernel_size == (3, 3) and conv.in_channels == cmid and dtype == torch.bfloat16 \
                        and ops.conv3x3_frag_supported(hw, hw, cmid, dtype)
                    convs.append(_TailConv(conv, bn, device, dtype, frag))
                state.append(convs)
            self._tail_state, self._tail_state_key = state, skey
            self.tail_grad_flat = None
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        k = self.tail_start()
        for i, convs in enumerate(self._tail_state):
            for tc in convs:
                tc.fold(stream)
            if len(convs) == 3:
                c1, c2, c3 = convs
                self._plan[k + i] = ("block", c1.folded(), c2.folded(), c3.folded(), None, None,
                                     (c2.frag, c2.b_fold) if c2.frag is not None else None)
            else:
                tc = convs[0]
                self._plan[k + i] = ("conv", tc.folded(), True, (tc.frag, tc.b_fold) if tc.frag is not None else None)

    def _attach_tail_grads(self):
        """Make the tail parameters' .grad views of ``tail_grad_flat`` (the decoder's rule, Decoder._attach_grads);
        return True if they already were: the backward then accumulates, else it overwrites."""
        params = self.tail_parameters()
        if self.tail_grad_flat is None or self.tail_grad_flat.device != params[0].device:
            total, off = 0, {}
            for p in params:
                off[p] = total
                total += (p.numel() + 63) // 64 * 64   # 256-byte aligned views
            self.tail_grad_flat = torch.zeros(total, device=params[0].device, dtype=torch.float32)
            for convs in self._tail_state:
                for tc in convs:
                    tc.offsets = {p: off[p] for p in tc.params()}
        attached = True
        base = self.tail_grad_flat
        for convs in self._tail_state:
            for tc in convs:
                for p, o in tc.offsets.items():
                    if p.grad is None or p.grad.data_ptr() != base.data_ptr() + 4 * o:
                        attached = False
                        p.grad = base[o:o + p.numel()].view(p.shape)
        return attached

    def _tail_unit_forward(self, y, step):
        """One unit of the tail as the plan runs it (separate c1 / c2 / c3 launches, layer4's form) -> (its output,
        the activations its backward needs: the forward's own tensors)."""
        if step[0] == "conv":
            out = self._run_step(y, step)[0]
            return out, (y, out)
        _, c1, c2, c3, ds, fused, c2f = step
        a1 = self._conv(y, c1, True)
        if c2f is not None and self.c2_frag and a1.shape[1] in self.c2_frag_sizes \
                and ops.conv3x3_frag_supported(a1.shape[1], a1.shape[2], a1.shape[3], a1.dtype):
            a2 = self._frag_conv("c2frag", ops.conv3x3_frag, a1, c2f)
        else:
            a2 = self._conv(a1, c2, True)
        out = self._conv(a2, c3, True, residual=y)
        return out, (y, a1, a2, out)

    def _launch(self, record, fn, *args, **kw):
        """One conv launch with the bench's hooks: its arguments recorded, an event pair around it,
        the in-graph launch timer's marks."""
        if self.timing_args is not None:
            self.timing_args.append(record)
        kw["policy"] = self.launch_policy() if self.launch_policy is not None else self.policy
        if self.timing is None:
            y = fn(*args, **kw)
        else:
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            y = fn(*args, **kw)
            en.record()
            self.timing.append((st, en))
        return y

    def _conv(self, x, f, relu, residual=None, out_hw=None):
        w, b, s, p = f
        return self._launch((x, w, b, s, p, relu, residual, out_hw), ops.conv2d_nhwc, x, w, b, s, p, relu,
                            residual=residual, out_hw=out_hw)

    def _stem(self, y, plan, stop, out_hw):
        """The space-to-depth stem on its input ``y`` and the rest of the plan up to ``stop``.  The pool step joins the
        stem's launch where ops.conv_stem_pool runs both; the stem keeps its one bench-hook record either way (the
        pool never had one)."""
        w, b, s, p = plan[0][1]
        pool = plan[1][1:] if len(plan) > 1 and plan[1][0] == "pool" else None
        if self.stem_pool and pool is not None and stop >= 2 \
                and ops.conv_stem_pool_supported(y, w, s, p, True, pool, out_hw, self.policy):
            y = self._launch((y, w, b, s, p, True, None, out_hw), ops.conv_stem_pool, y, w, b, s, p, True, pool,
                             out_hw=out_hw)
            return self._run_plan(y, plan, stop, 2)
        return self._run_plan(self._conv(y, plan[0][1], True, out_hw=out_hw), plan, stop)

    def _frag_conv(self, kind, fn, x, f, *extra):
        """A half-image fragment-weight conv launch (csrc/convblock.hip), with the bench's hooks."""
        return self._launch((kind, x, f) + extra, fn, x, f, *extra)

    # ---- plan: folded NHWC weights ------------------------------------------
    @torch.no_grad()
    def _fold(self, conv, bn, pad_in=None):
        w = conv.weight.detach().float()
        b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
        if bn is not None:  # eval-mode BatchNorm2d folded into the conv
            scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
            w = w * scale[:, None, None, None]
            b = bn.bias.float() + (b - bn.running_mean.float()) * scale
        w = w.permute(0, 2, 3, 1)   # [Cout, KH, KW, Cin]
        if pad_in is not None and w.shape[3] < pad_in:
            w = torch.nn.functional.pad(w, (0, pad_in - w.shape[3]))
        return (w.contiguous().to(self.compute_dtype), b.contiguous(), conv.stride[0], conv.padding[0])

    def _state_key(self, device, dtype):
        """The prefix part of the state key: every parameter and buffer outside the trainable tail (all of them when
        nothing is trainable).  The tail's part is _tail_key()."""
        tail = {id(t) for t in self._tail_tensors()}
        return (device, dtype, tuple(p._version for p in self.net.parameters() if id(p) not in tail),
                tuple(b._version for b in self.net.buffers() if id(b) not in tail))

    def _build_plan(self, device, dtype):
        self.compute_dtype = dtype
        plan = []
        mods = list(self.net.children())
        if self.network == "resnet152":
            w, b, _, _ = self._fold(mods[0], mods[1])
            plan.append(("stem_s2d", (stem_weight_s2d(w.float()).to(self.compute_dtype).contiguous(), b, 1, 2),
                         self._fold(mods[0], mods[1], IN_PAD)))
            plan.append(("pool", 3, 2, 1))
            for layer in mods[4:]:
                for blk in layer:
                    ds = self._fold(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None
                    fused = self._fused_weights(plan, blk, ds)
                    plan.append(("block", self._fold(blk.conv1, blk.bn1), self._fold(blk.conv2, blk.bn2),
                                 self._fold(blk.conv3, blk.bn3), ds, fused,
                                 fused[1] if fused is not None else self._c2_frag_weights(blk)))
        else:
            first = True
            hw = 224   # spatial size at this conv for the 224 x 224 input the plan assumes (forward checks the real one)
            for i, m in enumerate(mods):
                if isinstance(m, nn.Conv2d):
                    relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                    f = self._fold(m, None, IN_PAD if first else None)
                    plan.append(("conv", f, relu, self._conv_frag_weights(m, f, relu, hw)))
                    first = False
                elif isinstance(m, nn.MaxPool2d):
                    plan.append(("pool", m.kernel_size, m.stride, m.padding))
                    hw //= 2
        self._plan = plan

    def _fused_weights(self, plan, blk, ds):
        """Fragment-layout weights of an identity-residual bottleneck the fused kernel runs, else None."""
        if ds is not None or blk.conv2.stride[0] != 1 or self.compute_dtype != torch.bfloat16 \
                or not blk.conv1.weight.is_cuda:
            return None
        # spatial size at this block: the trunk halves it at each stride-2 step (224 input assumed
        # by the plan; forward checks the activation's real size before taking the fused path)
        cin, cmid = blk.conv1.in_channels, blk.conv1.out_channels
        hw = {256: 56, 512: 28, 1024: 14, 2048: 7}.get(cin)
        if hw is None or not ops.bottleneck_fused_supported(hw, hw, cin, cmid, self.compute_dtype):
            return None
        frags = []
        for conv, bn in ((blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)):
            w, b, _, _ = self._fold(conv, bn)
            frags.append((ops.mfma_frag_layout(w.reshape(w.shape[0], -1)), b))
        return tuple(frags)

    def _conv_frag_weights(self, conv, folded, relu, hw):
        """Fragment-layout weights of a VGG19 3x3 / stride-1 C -> C conv + ReLU that the staged-input kernel runs
        at its spatial size (sat_conv3x3_frag: the 14 x 14, 512 -> 512 block-5 convs), else None."""
        if not relu or conv.kernel_size != (3, 3) or conv.stride != (1, 1) or conv.padding != (1, 1) \
                or conv.in_channels != conv.out_channels or self.compute_dtype != torch.bfloat16 \
                or not conv.weight.is_cuda or not ops.conv3x3_frag_supported(hw, hw, conv.out_channels, self.compute_dtype):
            return None
        w, b = folded[0], folded[1]
        return ops.mfma_frag_layout(w.reshape(w.shape[0], -1)), b

    def _c2_frag_weights(self, blk):
        """Fragment-layout c2 weights of a stride-1 block whose 3x3 the band kernel runs (layer2), else None."""
        if blk.conv2.stride[0] != 1 or self.compute_dtype != torch.bfloat16 or not blk.conv2.weight.is_cuda:
            return None
        cmid = blk.conv2.out_channels
        hw = {64: 56, 128: 28, 256: 14, 512: 7}.get(cmid)
        if hw is None or not ops.conv3x3_frag_supported(hw, hw, cmid, self.compute_dtype):
            return None
        w, b, _, _ = self._fold(blk.conv2, blk.bn2)
        return ops.mfma_frag_layout(w.reshape(w.shape[0], -1)), b

    def compiled_plan(self, device, dtype, tail=True):
        """The plan for (device, dtype).  ``tail=False`` leaves a fine-tuned encoder's tail entries as they are: a
        forward that stops before tail_start() (the frozen prefix running ahead on a side stream) must not re-fold
        weights the optimiser may still be writing on another stream."""
        key = self._state_key(device, dtype)
        if self._plan is None or self._plan_key != key:
            self._build_plan(device, dtype)
            self._plan_key = key
            self._tail_key_done = None
        if tail and self._fine_tune and torch.device(device).type == "cuda":
            # a weight update of the tail re-folds the tail's entries only (HIP launches), always by sat_conv_fold:
            # train and eval forwards of a fine-tuned encoder read identical weights
            tkey = (self._tail_key(), device, dtype)
            if self._tail_key_done != tkey:
                self._refold_tail(device, dtype)
                self._tail_key_done = tkey
        return self._plan

    def stage_starts(self, device=None, dtype=None):
        """Plan indices where each ResNet stage (layer1..layer4) starts; [] for VGG19."""
        plan = self.compiled_plan(device or next(self.parameters()).device, dtype or self.compute_dtype)
        starts, prev = [], None
        for i, step in enumerate(plan):
            if step[0] == "block":
                cout = step[3][0].shape[0]   # c3's output channels: 256 / 512 / 1024 / 2048
                if cout != prev:
                    starts.append(i)
                    prev = cout
        return starts

    def forward(self, x, dtype=None, steps=None):
        """Images [B,3,H,W] -> features [B, L, D].  ``steps=(start, stop)`` runs a slice of the
        plan (stage_starts()): start > 0 takes the NHWC activation the previous slice returned,
        stop < len(plan) returns the NHWC activation instead of [B, L, D]."""
        packed = isinstance(x, PackedImages)
        L.require_device(x.pixels if packed else x)
        dtype = dtype or self.compute_dtype
        dev = (x.pixels if packed else x).device
        plan = self.compiled_plan(dev, dtype, tail=False)
        start, stop = steps if steps is not None else (0, len(plan))
        k = self.tail_start()
        if stop > k:   # the slice reads the tail's entries: re-fold them (on this stream) if their weights changed
            plan = self.compiled_plan(dev, dtype)
        if self._fine_tune and torch.is_grad_enabled() and stop == len(plan) and start < stop:
            # the frozen prefix as always, under no_grad; the tail through an autograd Function that keeps the
            # activations its backward needs
            first = max(start, k) - k
            if start < k:
                with torch.no_grad():
                    x = self._forward_plain(x, packed, dtype, plan, start, k)
            elif not x.is_contiguous():
                raise ValueError("Encoder: the tail's input must be a contiguous NHWC activation")
            return _TailFn.apply(x, self, first, *self.tail_parameters())
        return self._forward_plain(x, packed, dtype, plan, start, stop)

    def _forward_plain(self, x, packed, dtype, plan, start, stop):
        if packed:   # decoded uint8 images: resize + normalize straight into the first layer's layout
            if start > 0:
                raise ValueError("Encoder: packed images enter at plan step 0")
            if plan[0][0] == "stem_s2d":
                y = ops.images_to_input(x, L.IMG_S2D16, dtype)
                return self._stem(y, plan, stop, (y.shape[1], y.shape[2]))
            else:
                y = ops.images_to_input(x, L.IMG_NHWC, dtype, c_pad=IN_PAD)
            return self._run_plan(y, plan, stop)
        if start > 0:
            return self._run_plan(x, plan, stop, start)
        H, W = x.shape[2], x.shape[3]
        if plan[0][0] == "stem_s2d" and H % 2 == 0 and W % 2 == 0:
            return self._stem(ops.nchw_to_s2d(x, dtype), plan, stop, (H // 2, W // 2))
        elif plan[0][0] == "stem_s2d":   # odd image sizes: the stem on the 8-channel layout
            y = self._conv(ops.nchw_to_nhwc(x, IN_PAD, dtype), plan[0][2], True)
        else:
            y = ops.nchw_to_nhwc(x, IN_PAD, dtype)
        return self._run_plan(y, plan, stop)

    @staticmethod
    def _block_cin(step):
        return step[1][0].shape[3]   # c1's folded weight [Cout, 1, 1, Cin]

    def _fuse_this(self, plan, step):
        if self._block_cin(step) == 512:
            return bool(self.fuse_layer2)
        f = self.fuse_blocks
        if f is True or f is False:
            return f
        elig = [s for s in plan if s[0] == "block" and s[5] is not None and self._block_cin(s) != 512]
        return next(i for i, s in enumerate(elig) if s is step) % int(f) == 0

    def _run_plan(self, y, plan, stop, start=0):
        """Plan steps start .. stop - 1.  A chained c3 hands the next block's c1 output (x1) to the next step of
        this loop only: never past ``stop``, and a slice entered at ``start`` > 0 runs its own first c1."""
        steps = [s for s in plan[start:stop] if s[0] != "stem_s2d"]
        x1 = None
        for i, step in enumerate(steps):
            y, x1 = self._run_step(y, step, x1, steps[i + 1] if i + 1 < len(steps) else None)
        if stop < len(plan):
            return y
        B, H, W, C = y.shape
        return y.view(B, H * W, C)

    def _block_fused(self, step, shape, dtype):
        """The block runs as ONE fused launch on an input of this NHWC shape."""
        return (step[5] is not None and self._fuse_this(self._plan, step)
                and ops.bottleneck_fused_supported(shape[1], shape[2], shape[3], step[1][0].shape[0], dtype))

    def _block_c1_frag(self, step, shape, dtype):
        return step[5] is not None and self.c1_frag and ops.conv1x1_frag_supported(shape[1], shape[2], shape[3],
                                                                                step[1][0].shape[0], dtype)

    def _chain_into(self, out, c3, nxt):
        """The c1 weights of the next plan step when this block's c3 (input ``out``) is launched chained with it."""
        if nxt is None or nxt[0] != "block" or out.shape[3] not in self.chain_c1:
            return None
        c1n = nxt[1]
        yshape = (out.shape[0], out.shape[1], out.shape[2], c3[0].shape[0])
        if c1n[2] != 1 or c1n[3] != 0 or c1n[0].shape[3] != yshape[3] or self._block_fused(nxt, yshape, out.dtype) \
                or self._block_c1_frag(nxt, yshape, out.dtype):
            return None
        if not ops.conv1x1_chain_supported(out.shape[0] * out.shape[1] * out.shape[2], out.shape[3], yshape[3],
                                           c1n[0].shape[0], out.dtype, self.policy):
            return None
        return c1n

    def _proj_into(self, y, out, c3, ds, c1n):
        """The block's projected residual when its c3 (input ``out``, chained into ``c1n`` or not) computes the
        downsample conv ``ds`` of the block input ``y`` inside its own launch, else None."""
        if ds is None or not {64: self.proj_l1, 128: self.proj_l2}.get(out.shape[3], False):
            return None
        proj = ops.ProjectedResidual(y, ds)
        if ds[3] != 0 or y.shape[0] != out.shape[0] or proj.out_hw() != (out.shape[1], out.shape[2]) \
                or tuple(ds[0].shape) != (c3[0].shape[0], 1, 1, y.shape[3]) \
                or y.numel() * y.element_size() >= 1 << 31 or not (y.is_contiguous() and out.is_contiguous()):
            return None
        if not ops.conv1x1_proj_supported(out.shape[0] * out.shape[1] * out.shape[2], out.shape[3], c3[0].shape[0],
                                          y.shape[3], ds[2], c1n[0].shape[0] if c1n is not None else 0, out.dtype,
                                          self.policy):
            return None
        return proj

    def _absorbed(self, y, f, relu=True):
        """The bench hooks of a launch that another launch already stands for (a c1 the previous block's chained c3
        computed, a downsample conv its block's c3 computes): its record in launch order, an empty event pair and one
        launch-policy slot, so per-launch tables keep their length."""
        w, b, s, p = f
        if self.timing_args is not None:
            self.timing_args.append((y, w, b, s, p, relu, None, None))
        if self.launch_policy is not None:
            self.launch_policy()
        if self.timing is not None:
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            en.record()
            self.timing.append((st, en))

    def _run_step(self, y, step, x1=None, nxt=None):
        """One plan step on activation y -> (its output, the next block's c1 output when this step's c3 was launched
        chained with it (``nxt``: the next step of the same forward), else None).  ``x1``: this block's c1 output
        handed over by the previous step."""
        if step[0] == "conv":
            f = step[3]
            if f is not None and self.c2_frag and y.shape[1] in self.c2_frag_sizes \
                    and ops.conv3x3_frag_supported(y.shape[1], y.shape[2], y.shape[3], y.dtype):
                return self._frag_conv("c2frag", ops.conv3x3_frag, y, f), None
            return self._conv(y, step[1], step[2]), None
        if step[0] == "pool":
            return ops.maxpool2d_nhwc(y, step[1], step[2], step[3]), None
        _, c1, c2, c3, ds, fused, c2f = step
        if x1 is not None:   # computed by the previous block's chained c3 launch (_chain_into ruled the other forms out)
            self._absorbed(y, c1)
            out = x1
        elif self._block_fused(step, y.shape, y.dtype):
            return self._launch(("fused", y, fused), ops.bottleneck_fused, y, *fused), None
        elif self._block_c1_frag(step, y.shape, y.dtype):
            out = self._frag_conv("c1frag", ops.conv1x1_frag, y, fused[0])
        else:
            out = self._conv(y, c1, True)
        if c2f is not None and self.c2_frag and out.shape[1] in self.c2_frag_sizes \
                and ops.conv3x3_frag_supported(out.shape[1], out.shape[2], out.shape[3],
                                                                         out.dtype):
            out = self._frag_conv("c2frag", ops.conv3x3_frag, out, c2f)
        else:
            out = self._conv(out, c2, True)
        c1n = self._chain_into(out, c3, nxt)
        idn = self._proj_into(y, out, c3, ds, c1n)
        if idn is not None:   # the downsample launch's record keeps its place: after c2, before c3
            self._absorbed(y, ds, False)
        else:
            idn = self._conv(y, ds, False) if ds is not None else y
        if c1n is not None:
            w, b, s, p = c3
            return self._launch((out, w, b, s, p, True, idn, None), ops.conv1x1_chain, out, c3, idn, c1n)
        return self._conv(out, c3, True, residual=idn), None

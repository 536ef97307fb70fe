"""Integer-valued cases on which every GEMM / conv kernel has exactly one right output bit pattern.

Operands are integers times one power of two per layer, with every partial sum below 2^24 in units of the layer's
quantum.  Every product and every partial sum is then exact in fp32 (the fp32 MFMA, and the bf16 MFMA with fp32
accumulation), so the result does not depend on tile shape, k order, split-K order or atomics: it is the fp64 result,
rounded to nearest-even once where the output is bf16.  tests/test_gpu_exact.py compares each kernel with that
reference by torch.equal; tests/test_cpu_exact_cases.py proves on the CPU that every case meets the conditions below
and that four deliberately wrong references (MUTANTS) differ from the true one.  No GPU use here.

Regimes
  small     max |out| <= 256 quanta at every bf16 tensor: every output is bf16-representable, so any single dropped or
            added product changes an output.
  rounding  at least 1 % of the bf16 outputs are exact ties (low 16 bits of the fp32 value = 0x8000), and with a
            residual max |conv + bias| > 256 quanta, so rounding before the residual add is visible.
  exact     no sum at all (max pool): the output is one of the inputs.

Fused and chained entry points round to bf16 exactly where the separate launches would write a bf16 tensor (DESIGN
4.11 / 4.13 and the kernels' contracts in include/sat_hip.h): the downsample output before the residual add, the c1
and c2 outputs of the fused bottleneck, y before the chained c1, the stem conv's output before the pool.
"""
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

BF, F32 = torch.bfloat16, torch.float32
LIMIT = float(1 << 24)
MUTANTS = ("drop", "trunc", "away", "early")

# id, kernel family, regime, p: the problem (hashable; cases that differ only in ``pol`` share one reference),
# pol: SatPolicy fields of the call
Case = namedtuple("Case", "id family regime p pol")


# ---------------------------------------------------------------------------- bf16 rounding, three ways
def round_bf16(v, mode="rne"):
    """fp64 / fp32 values that fit fp32 -> bf16, rounding to nearest-even ("rne"), toward zero ("trunc") or half away
    from zero ("away"), on the fp32 bit pattern."""
    f = v.float()
    assert torch.equal(f.double(), v.double()), "the value does not fit fp32: the rounding would not be a single one"
    b = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if mode == "rne":
        b = b + 0x7FFF + ((b >> 16) & 1)
    elif mode == "away":
        b = b + 0x8000
    elif mode != "trunc":
        raise ValueError(mode)
    b = b & 0xFFFF0000
    b = torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32)
    return b.view(torch.float32).bfloat16()   # the low 16 bits are zero: this conversion is exact


def is_tie(v):
    """Which fp32 values lie exactly between two bf16 values."""
    return (v.float().contiguous().view(torch.int32) & 0xFFFF) == 0x8000


# ---------------------------------------------------------------------------- generators
def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def ints(g, shape, a):
    """Uniform integers in [-a, a] as fp64."""
    return torch.randint(-a, a + 1, tuple(shape), generator=g).double()


def ternary(g, shape, density):
    """{-1, 0, 1} as fp64, nonzero with probability ``density``."""
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return sign * (torch.rand(tuple(shape), generator=g) < density).double()


def operand_ranges(regime, K):
    """(activation range or 0 = ternary, weight range or 0 = ternary, weight density, |bias|, |residual|) in quanta.
    small: the sum's deviation stays near 20 whatever K (K x density <= 576); rounding: dense operands whose sum's
    deviation is 250-750, so a good part of the outputs lies above 256 where odd integers are ties."""
    if regime == "small":
        return 0, 0, min(0.5, 576.0 / K), 4, 16
    if K >= 2048:
        return 4, 2, 1.0, 4, 64
    if K >= 512:
        return 8, 4, 1.0, 4, 64
    return 16, 8, 1.0, 4, 64


def make_x(g, shape, regime, K):
    ax = operand_ranges(regime, K)[0]
    return ints(g, shape, ax) if ax else ternary(g, shape, 2.0 / 3.0)


def make_w(g, shape, regime, K, density=None):
    _, aw, d, _, _ = operand_ranges(regime, K)
    return ints(g, shape, aw) if aw else ternary(g, shape, density or d)


# ---------------------------------------------------------------------------- linear maps, fp64 (or fp32 for bounds)
def mm(A, B):
    """A [M,K] x B [N,K] -> [M,N]."""
    return A @ B.T


def conv(x, w, stride=1, pad=0, out_hw=None):
    """x NCHW, w OIHW; ``pad`` pads top / left, ``out_hw`` fixes the output size (bottom / right padding = whatever
    it implies), as sat_conv2d_nhwc defines it."""
    H, W = x.shape[2:]
    KH, KW = w.shape[2:]
    if out_hw is None:
        out_hw = ((H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1)
    pb = max(0, (out_hw[0] - 1) * stride + KH - H - pad)
    pr = max(0, (out_hw[1] - 1) * stride + KW - W - pad)
    y = F.conv2d(F.pad(x, (pad, pr, pad, pb)), w, stride=stride)
    return y[:, :, :out_hw[0], :out_hw[1]]


def im2col3x3(x):
    """x [N,H,W,C] -> [N H W, 9 C], column (kh 3 + kw) C + c = x[n, oh + kh - 1, ow + kw - 1, c] (zero outside)."""
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    cols = [xp[:, kh:kh + H, kw:kw + W, :] for kh in range(3) for kw in range(3)]
    return torch.stack(cols, dim=3).reshape(N * H * W, 9 * C)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------- one stage and its conditions
class Built:
    """A case's operands (``args``: CPU tensors in the layout and dtype the entry point takes), the expected outputs
    (``outs``), and what the conditions and mutants need."""

    def __init__(self, case):
        self.case = case
        self.args, self.outs = {}, {}
        self.stages = []       # (name, max partial-sum bound in quanta or None, max |out| in quanta, bf16 output)
        self.final = None      # the stage the mutants are applied to
        self.post = None       # final stage's output -> the entry point's outputs (a later stage, the pool)


def _fits(t, dtype, what):
    assert torch.equal(t.to(dtype).double(), t), f"{what}: not representable in {dtype}"


def stage(b, name, lin, x, w, q, bias=None, res=None, relu=False, dtype=BF, stats=False, product=None, final=False):
    """out = dtype(act(lin(x, w) + bias + res)) with every value a multiple of the quantum ``q``; records the
    conditions' figures and, for the final stage, what the mutants need.  ``bias`` broadcasts against the sum;
    ``product``: (m, n) -> the products x * w that enter output element (m, n) of ``lin``, flattened."""
    acc = lin(x, w)
    v = acc if bias is None else acc + bias
    pre_res = v
    if res is not None:
        v = v + res
    if relu:
        v = v.clamp_min(0)
    assert torch.equal(v.float().double(), v), f"{name}: the fp64 value does not fit fp32"
    assert torch.equal((v / q).round() * q, v), f"{name}: not a multiple of the quantum"
    out = round_bf16(v) if dtype == BF else v.float()
    bound = None
    if stats:   # nonnegative integers below 2^24 add exactly in fp32, and a sum that reaches 2^24 never falls below it
        bound = lin(x.abs().float(), w.abs().float()).double()
        for t in (bias, res):
            if t is not None:
                bound = bound + t.abs()
        bound = (bound / q).max().item()
    b.stages.append((name, bound, (v.abs() / q).max().item(), dtype == BF))
    if final:
        b.final = dict(name=name, acc=acc, bias=bias, res=res, relu=relu, dtype=dtype, q=q, pre=v,
                       conv_max=(pre_res.abs() / q).max().item(), product=product)
    return out


def mutant(b, kind):
    """The final stage computed wrongly -> the entry point's outputs (as ``b.outs``).  drop: one product removed from
    one output; trunc: truncation instead of rounding; away: round-half-away; early: the sum rounded to bf16 before the
    residual is added."""
    f = b.final
    acc = f["acc"]
    if kind == "drop":
        # at the largest output (it survives a ReLU, and a pool window), remove a negative product: the output rises
        # (with a pool after it, only the largest output is sure to be seen: there the first candidate has to do)
        flat = f["pre"].reshape(-1)
        for i in flat.topk(1 if b.case.family == "stempool" else min(64, flat.numel())).indices.tolist():
            pos = tuple(int(j) for j in np.unravel_index(i, tuple(f["pre"].shape)))
            prods = f["product"](pos)
            neg = prods[prods < 0]
            if neg.numel() > 0:
                break
        assert neg.numel() > 0, "no negative product at the largest outputs"
        acc = acc.clone()
        acc[pos] -= neg[0]
    v = acc if f["bias"] is None else acc + f["bias"]
    if kind == "early":
        assert f["res"] is not None and f["dtype"] == BF
        v = round_bf16(v).double()
    if f["res"] is not None:
        v = v + f["res"]
    if f["relu"]:
        v = v.clamp_min(0)
    mode = {"trunc": "trunc", "away": "away"}.get(kind, "rne")
    out = round_bf16(v, mode) if f["dtype"] == BF else v.float()
    return b.post(out)


def applicable_mutants(b):
    """drop on every small-regime case; the rounding mutants on every rounding-regime case with bf16 output (early
    rounding only where there is a residual to add after it)."""
    if b.final is None:
        return ()
    if b.case.regime == "small":
        return ("drop",)
    if b.final["dtype"] != BF:
        return ()
    return ("trunc", "away") + (("early",) if b.final["res"] is not None else ())


def check_conditions(b):
    """The per-case conditions of the module docstring; ``b`` built with stats."""
    regime = b.case.regime
    for name, bound, outq, is_bf in b.stages:
        assert bound is not None and bound < LIMIT, (b.case.id, name, "partial sums reach 2^24", bound)
        if regime == "small" and is_bf:
            assert outq <= 256, (b.case.id, name, "max |out| above 256 quanta", outq)
    f = b.final
    if regime == "rounding" and f is not None and f["dtype"] == BF:
        ties = is_tie(f["pre"]).double().mean().item()
        assert ties >= 0.01, (b.case.id, "ties", ties)
        if f["res"] is not None:
            assert f["conv_max"] > 256, (b.case.id, "max |conv| <= 256 quanta", f["conv_max"])
    return b


def figures(b):
    """One line of the case's figures, for the record."""
    f = b.final
    ties = is_tie(f["pre"]).double().mean().item() if f is not None and f["dtype"] == BF else float("nan")
    st = ", ".join(f"{n}: bound {bd:.0f} max|out| {o:.0f}" for n, bd, o, _ in b.stages)
    return f"{b.case.id}: ties {100 * ties:.1f} %; {st}"


# ---------------------------------------------------------------------------- builders, one per kind of problem
def _mm_product(A, B):
    return lambda pos: A[pos[0]] * B[pos[1]]


def _conv_product(x, w, stride, pad):
    """Products entering output (n, co, oh, ow) of conv(x, w, stride, pad): the window of the zero-padded input."""
    KH, KW = w.shape[2:]
    xp = F.pad(x, (pad, KW, pad, KH))   # enough zeros bottom / right for any out_hw

    def prods(pos):
        n, co, oh, ow = pos
        return (xp[n, :, oh * stride:oh * stride + KH, ow * stride:ow * stride + KW] * w[co]).reshape(-1)
    return prods


def build_gemm(b, p, regime, stats):
    """sat_gemm: C = act(A' B'^T + bias + add1 + beta C)."""
    M, N, K = p["M"], p["N"], p["K"]
    dt, cdt = p["dtype"], p["cdt"]
    g = _gen("gemm", M, N, K, regime)
    q = 2.0 ** p.get("sw", -3 if regime == "small" else -8)
    _, _, _, ab, ar = operand_ranges(regime, K)
    A = make_x(g, (M, K), regime, K)
    B = make_w(g, (N, K), regime, K) * q
    bias = ints(g, (N,), ab) * q if p.get("bias") else None
    add1 = ints(g, (M, N), ar) * q if p.get("add1") is not None else None
    C0 = ints(g, (M, N), 16) * q if p.get("beta") else None
    for t, d, n in ((A, dt, "A"), (B, dt, "B"), (add1, p.get("add1"), "add1")):
        if t is not None:
            _fits(t, d, n)
    res = None
    if add1 is not None or C0 is not None:
        res = (add1 if add1 is not None else 0) + (p["beta"] * C0 if C0 is not None else 0)
    out = stage(b, "C", mm, A, B, q, bias, res, p.get("relu", False), cdt, stats, _mm_product(A, B), final=True)
    b.args = dict(A=(A.T.contiguous() if p["tA"] else A).to(dt), B=(B.T.contiguous() if p["tB"] else B).to(dt),
                  bias=None if bias is None else bias.float(), add1=None if add1 is None else add1.to(p["add1"]),
                  C0=None if C0 is None else C0.to(cdt))
    aux = p.get("aux")
    pre = b.final["pre"]

    def post(o):
        return {"C": o, "aux": (round_bf16(pre) if aux == BF else pre.float())} if aux is not None else {"C": o}
    b.post = post
    b.outs = post(out)


def build_conv(b, p, regime, stats):
    """sat_conv2d_nhwc (and the fragment kernels): y = act(conv(x, w) + bias + residual), optionally max-pooled."""
    N, C, H, W, Cout = p["N"], p["C"], p["H"], p["W"], p["Cout"]
    KH, KW = p["k"] if isinstance(p["k"], tuple) else (p["k"], p["k"])
    stride, pad, out_hw = p.get("stride", 1), p.get("pad", 0), p.get("out_hw")
    dt = p.get("dtype", BF)
    K = KH * KW * C
    g = _gen("conv", N, C, H, W, Cout, KH, stride, pad, regime)
    q = 2.0 ** p.get("sw", -3 if regime == "small" else -8)
    _, _, _, ab, ar = operand_ranges(regime, K)
    x = make_x(g, (N, C, H, W), regime, K)
    w = make_w(g, (Cout, C, KH, KW), regime, K) * q
    bias = ints(g, (1, Cout, 1, 1), ab) * q if p.get("bias", True) else None
    lin = lambda a, c: conv(a, c, stride, pad, out_hw)   # noqa: E731
    shape = lin(x[:1, :1], w[:1, :1]).shape[2:]
    res = ints(g, (N, Cout) + tuple(shape), ar) * q if p.get("res") else None
    for t, n in ((x, "x"), (w, "w"), (res, "res")):
        if t is not None:
            _fits(t, dt, n)
    out = stage(b, "y", lin, x, w, q, bias, res, p.get("relu", False), dt, stats, _conv_product(x, w, stride, pad),
                final=True)
    b.args = dict(x=nhwc(x).to(dt), w=nhwc(w).to(dt), bias=None if bias is None else bias.reshape(-1).float(),
                  res=None if res is None else nhwc(res).to(dt))
    pool = p.get("pool")

    def post(o):
        if pool is not None:
            o = F.max_pool2d(o.float(), *pool).to(o.dtype)
        return {"y": nhwc(o)}
    b.post = post
    b.outs = post(out)


def _w1x1(g, cout, cin, regime, q, density=None):
    return make_w(g, (cout, cin), regime, cin, density) * q


def build_chain(b, p, regime, stats):
    """sat_conv1x1_chain / sat_conv1x1_proj: y = relu(x w^T + b + residual), residual given or
    bf16(xin_strided wp^T + bp); x1 = relu(y w1^T + b1) when N2 > 0.  y is the bf16 tensor the c1 reads."""
    K, Nc, N2, Kp, S = p["K"], p["N"], p.get("N2", 0), p.get("Kp", 0), p.get("S", 1)
    Bn, H, W = p["B"], p["H"], p["W"]
    M = Bn * H * W
    g = _gen("chain", K, Nc, N2, Kp, S, M, regime)
    small = regime == "small"
    q = 2.0 ** (-2 if small else -8)
    _, _, _, ab, ar = operand_ranges(regime, K)
    x = make_x(g, (M, K), regime, K)
    w = _w1x1(g, Nc, K, regime, q)
    bias = ints(g, (Nc,), ab) * q
    b.args = dict(x=x.reshape(Bn, H, W, K).to(BF), w=w.reshape(Nc, 1, 1, K).to(BF), bias=bias.float())
    if Kp:   # the projection shortcut: its output is rounded to bf16 before the add, as its own launch would
        xin = make_x(g, (Bn, S * H, S * W, Kp), regime, Kp)
        wp = _w1x1(g, Nc, Kp, regime, q)
        bp = ints(g, (Nc,), ab) * q
        res = stage(b, "downsample", mm, xin[:, ::S, ::S, :].reshape(M, Kp), wp, q, bp, None, False, BF, stats).double()
        b.args.update(xin=xin.to(BF), wp=wp.reshape(Nc, 1, 1, Kp).to(BF), bp=bp.float())
    else:
        res = ints(g, (M, Nc), ar) * q
        b.args.update(res=res.reshape(Bn, H, W, Nc).to(BF))
    y = stage(b, "y", mm, x, w, q, bias, res, True, BF, stats, _mm_product(x, w), final=True)
    if N2:
        # the c1 reads the rounded y (multiples of q); small: few enough taps that its outputs stay below 256 quanta
        q1 = q * 2.0 ** (-1 if small else -6)
        w1 = _w1x1(g, N2, Nc, regime, q1 / q, density=16.0 / Nc) if small else ints(g, (N2, Nc), 2) * (q1 / q)
        b1 = ints(g, (N2,), ab) * q1
        b.args.update(w1=w1.reshape(N2, 1, 1, Nc).to(BF), b1=b1.float())

    def post(o):
        outs = {"y": o.reshape(Bn, H, W, Nc)}
        if N2:
            outs["x1"] = stage(Built(b.case), "x1", mm, o.double(), w1, q1, b1, None, True, BF).reshape(Bn, H, W, N2)
        return outs
    if N2:   # once with the conditions' figures
        stage(b, "x1", mm, y.double(), w1, q1, b1, None, True, BF, stats)
    b.post = post
    b.outs = post(y)


def build_block(b, p, regime, stats):
    """sat_bottleneck_fused: y = relu(c3(relu(c2(relu(c1(x))))) + x); the c1 and c2 outputs are bf16 tensors of the
    three launches it replaces.  Each layer's weights carry a power-of-two scale of their own (the stage quanta q1, q2,
    q3); small: a negative bias and few taps keep every stage below 256 quanta."""
    N, H, C, Cm = p["N"], p["H"], p["C"], p["Cmid"]
    g = _gen("block", N, H, C, Cm, regime)
    small = regime == "small"
    x = ternary(g, (N, C, H, H), 0.5).abs() if small else ints(g, (N, C, H, H), 4).clamp_min(0)   # a block input: >= 0
    # the residual x (quantum 1) is added to c3's sum (quantum q3): x / q3 has to stay a small integer too
    q1 = 2.0 ** (-1 if small else -2)
    q2 = q1 * 0.5
    q3 = q2 * 0.5
    if small:
        w1 = ternary(g, (Cm, C, 1, 1), 128.0 / C) * q1
        w2 = ternary(g, (Cm, Cm, 3, 3), 8.0 / Cm) * (q2 / q1)
        w3 = ternary(g, (C, Cm, 1, 1), 8.0 / Cm) * (q3 / q2)
        b1, b2, b3 = (ints(g, (1, Cm, 1, 1), 2) - 8) * q1, (ints(g, (1, Cm, 1, 1), 2) - 16) * q2, \
            ints(g, (1, C, 1, 1), 4) * q3
    else:
        w1 = ints(g, (Cm, C, 1, 1), 2) * q1
        w2 = ints(g, (Cm, Cm, 3, 3), 1) * (q2 / q1)
        w3 = ints(g, (C, Cm, 1, 1), 1) * (q3 / q2)
        b1, b2, b3 = ints(g, (1, Cm, 1, 1), 4) * q1, ints(g, (1, Cm, 1, 1), 4) * q2, ints(g, (1, C, 1, 1), 4) * q3
    for t, n in ((x, "x"), (w1, "w1"), (w2, "w2"), (w3, "w3")):
        _fits(t, BF, n)
    c1 = lambda a, c: conv(a, c)            # noqa: E731
    c2 = lambda a, c: conv(a, c, 1, 1)      # noqa: E731
    t1 = stage(b, "c1", c1, x, w1, q1, b1, None, True, BF, stats).double()
    t2 = stage(b, "c2", c2, t1, w2, q2, b2, None, True, BF, stats).double()
    # the residual x is a multiple of q3 as well (q3 divides 1)
    y = stage(b, "c3", c1, t2, w3, q3, b3, x, True, BF, stats, _conv_product(t2, w3, 1, 0), final=True)
    b.args = dict(x=nhwc(x).to(BF), w1=nhwc(w1).to(BF), b1=b1.reshape(-1).float(), w2=nhwc(w2).to(BF),
                  b2=b2.reshape(-1).float(), w3=nhwc(w3).to(BF), b3=b3.reshape(-1).float())
    b.post = lambda o: {"y": nhwc(o)}
    b.outs = b.post(y)


def build_pool(b, p, regime, stats):
    """sat_maxpool2d_nhwc: the output is one of the inputs."""
    N, C, H, W = p["N"], p["C"], p["H"], p["W"]
    g = _gen("pool", N, C, H, W)
    x = (ints(g, (N, C, H, W), 200) * 0.25).to(p["dtype"])
    b.args = dict(x=nhwc(x))
    b.outs = {"y": nhwc(F.max_pool2d(x.float(), *p["pool"]).to(p["dtype"]))}


def build_wgrad(b, p, regime, stats):
    """sat_conv3x3_wgrad: dw[co][kh][kw][ci] (+)= sum over pixels of dz x, fp32."""
    N, H, W, Cin, Cout = p["N"], p["H"], p["W"], p["Cin"], p["Cout"]
    g = _gen("wgrad", N, H, W, Cin, Cout)
    x = ternary(g, (N, H, W, Cin), 2.0 / 3.0)
    dz = ternary(g, (N, H, W, Cout), 0.5) * 0.5
    prior = ints(g, (Cout, 9 * Cin), 16) * 0.5 if p.get("accumulate") else None
    cols, dz2 = im2col3x3(x).T.contiguous(), dz.reshape(-1, Cout).T.contiguous()   # [9 Cin, K], [Cout, K]
    out = stage(b, "dw", mm, dz2, cols, 0.5, None, prior, False, F32, stats, _mm_product(dz2, cols), final=True)
    b.args = dict(x=x.to(p["dtype"]), dz=dz.to(p["dtype"]),
                  prior=None if prior is None else prior.reshape(Cout, 3, 3, Cin).float())
    b.post = lambda o: {"dw": o.reshape(Cout, 3, 3, Cin)}
    b.outs = b.post(out)


BUILDERS = dict(gemm=build_gemm, conv=build_conv, chain=build_chain, block=build_block, pool=build_pool,
                wgrad=build_wgrad)
_CACHE = {}


def build(case, stats=False):
    """The case's operands and reference, computed once per problem (cases that differ only in policy share it)."""
    key = (case.regime, case.p, stats)
    hit = _CACHE.get(key) or _CACHE.get((case.regime, case.p, True))
    if hit is None:
        p = dict(case.p)
        hit = Built(case)
        BUILDERS[p["kind"]](hit, p, case.regime, stats)
        _CACHE[key] = hit
    if hit.case is not case:   # the shared reference under this case's name
        twin = Built(case)
        twin.__dict__.update({k: v for k, v in hit.__dict__.items() if k != "case"})
        return twin
    return hit


# ---------------------------------------------------------------------------- the case table
def _p(kind, **kw):
    return tuple(sorted(dict(kind=kind, **kw).items(), key=lambda kv: kv[0]))


def _pol(**kw):
    return tuple(sorted(kw.items()))


def _both(cases, cid, family, p, pol=()):
    for regime in ("small", "rounding"):
        cases.append(Case(f"{cid}-{regime}", family, regime, p, pol))


def _table():
    cs = []
    lay = {(False, False): "NN", (False, True): "NT", (True, False): "TN", (True, True): "TT"}

    # gemm_kernel (gemm.hip): fp32 operands always; bf16 operands where the LDS-DMA kernel refuses (K % 8 != 0, aux)
    for (tA, tB), nm in lay.items():
        cs.append(Case(f"gemm-f32-{nm}-37x45x29", "gemm", "small",
                       _p("gemm", M=37, N=45, K=29, tA=tA, tB=tB, dtype=F32, cdt=F32, bias=True, add1=F32, relu=True), ()))
        cs.append(Case(f"gemm-f32-{nm}-130x257x200-aux", "gemm", "small",
                       _p("gemm", M=130, N=257, K=200, tA=tA, tB=tB, dtype=F32, cdt=F32, bias=True, add1=BF, relu=True,
                          aux=BF), ()))
        _both(cs, f"gemm-bf16-{nm}-37x45x29", "gemm",
              _p("gemm", M=37, N=45, K=29, tA=tA, tB=tB, dtype=BF, cdt=BF, bias=True, add1=F32, relu=True))
        _both(cs, f"gemm-bf16-{nm}-130x257x200-aux", "gemm",
              _p("gemm", M=130, N=257, K=200, tA=tA, tB=tB, dtype=BF, cdt=BF, bias=True, add1=BF, relu=True, aux=F32))
    cs.append(Case("gemm-f32-beta1", "gemm", "small",
                   _p("gemm", M=37, N=45, K=29, tA=False, tB=False, dtype=F32, cdt=F32, beta=1.0), ()))
    cs.append(Case("gemm-bf16-beta1", "gemm", "small",
                   _p("gemm", M=130, N=257, K=204, tA=False, tB=True, dtype=BF, cdt=F32, beta=1.0), ()))
    # enough tiles for the generic kernel's 64 x 128 (>= 240 of them) and 128 x 128 tile shapes
    for M, nm in [(1000, "64x128"), (2040, "128x128")]:
        cs.append(Case(f"gemm-f32-NT-tiles{nm}", "gemm", "small",
                       _p("gemm", M=M, N=1930, K=29, tA=False, tB=True, dtype=F32, cdt=F32, bias=True, relu=True), ()))
        _both(cs, f"gemm-bf16-NN-tiles{nm}", "gemm",
              _p("gemm", M=M, N=1930, K=29, tA=False, tB=False, dtype=BF, cdt=BF, bias=True, relu=True))
    # ... and as an fp32 conv (implicit im2col): the parity path of the trunk
    for cid, kw in [("3x3", dict(N=2, C=8, H=15, W=11, Cout=16, k=3, pad=1)),
                    ("1x1-s2", dict(N=2, C=16, H=16, W=12, Cout=24, k=1, stride=2)),
                    ("7x7-s2", dict(N=1, C=8, H=20, W=16, Cout=64, k=7, stride=2, pad=3))]:
        cs.append(Case(f"gemm-f32-conv-{cid}", "gemm", "small", _p("conv", dtype=F32, relu=True, res=True, **kw), ()))
    for beta in (0.0, 1.0):   # few tiles, K >= 256, fp32 C, no epilogue: the generic kernel's atomic split-K
        cs.append(Case(f"gemm-bf16-atomic-beta{int(beta)}", "gemm", "small",
                       _p("gemm", M=64, N=72, K=260, tA=False, tB=False, dtype=BF, cdt=F32, beta=beta), ()))

    # fast_gemm_kernel (convgemm.hip) as a GEMM: every tile configuration, ring depth, epilogue and tile order
    off = dict(conv_pipe=1, conv_stream=1, conv3x3_ws=1, split_gemm=1, skinny=1)
    nt = dict(tA=False, tB=False, dtype=BF, bias=True, relu=True)
    for tile in (1, 2, 3, 4, 5):
        for stages in ((2, 3) if tile in (1, 2, 3) else (2,)):   # the 256-wide and 256-high tiles have one depth
            _both(cs, f"fast-tile{tile}-stages{stages}", "fast",
                  _p("gemm", M=300, N=200, K=320, cdt=BF, add1=BF, **nt), _pol(gemm_tile=tile, gemm_stages=stages, **off))
    cs.append(Case("fast-tile1-f32out", "fast", "small", _p("gemm", M=300, N=200, K=320, cdt=F32, add1=F32, **nt),
                   _pol(gemm_tile=1, **off)))
    for epi in (0, 1, 2):   # N a multiple of the tile width: the bf16 LDS epilogue is eligible
        for add1 in (BF, None):
            _both(cs, f"fast-epilogue{epi}-{'res' if add1 else 'plain'}", "fast",
                  _p("gemm", M=300, N=256, K=320, cdt=BF, add1=add1, **nt), _pol(gemm_epilogue=epi, **off))
    for add1 in (BF, None):   # the LDS epilogue on 128 x 128 tiles (unforced, these few tiles run 128 x 64)
        _both(cs, f"fast-epilogue0-tile1-{'res' if add1 else 'plain'}", "fast",
              _p("gemm", M=300, N=256, K=320, cdt=BF, add1=add1, **nt), _pol(gemm_tile=1, **off))
    _both(cs, "fast-linear-order", "fast", _p("gemm", M=300, N=200, K=320, cdt=BF, add1=BF, **nt),
          _pol(gemm_linear_order=1, **off))
    for (tA, tB), nm in lay.items():   # the k-major operand forms
        if tA or tB:
            cs.append(Case(f"fast-{nm}-f32out", "fast", "small",
                           _p("gemm", M=304, N=200, K=320, tA=tA, tB=tB, dtype=BF, cdt=F32, bias=True), _pol(**off)))
            _both(cs, f"fast-{nm}", "fast",
                  _p("gemm", M=304, N=200, K=320, tA=tA, tB=tB, dtype=BF, cdt=BF, bias=True, add1=BF, relu=True),
                  _pol(**off))
    for cid, tA, tB, pol in [("TT-tile3", True, True, dict(gemm_tile=3)), ("NT-stages3", False, True, dict(gemm_stages=3)),
                             ("TN-tile3-stages3", True, False, dict(gemm_tile=3, gemm_stages=3))]:
        _both(cs, f"fast-{cid}", "fast",
              _p("gemm", M=304, N=200, K=320, tA=tA, tB=tB, dtype=BF, cdt=BF, bias=True, add1=BF, relu=True),
              _pol(**pol, **off))
    for beta in (0.0, 1.0):   # atomic split-K: K >= 1024 and few tiles
        cs.append(Case(f"fast-atomic-NN-beta{int(beta)}", "fast", "small",
                       _p("gemm", M=300, N=136, K=1104, tA=False, tB=False, dtype=BF, cdt=F32, beta=beta), _pol(**off)))
        cs.append(Case(f"fast-atomic-TT-beta{int(beta)}", "fast", "small",
                       _p("gemm", M=256, N=136, K=1024, tA=True, tB=True, dtype=BF, cdt=F32, beta=beta), _pol(**off)))
    # ... and as a conv: uniform taps (C % 64 == 0), per-lane taps (C = 32, 16, 8), stride 2, H != W, out_hw
    for cid, kw in [("c64-3x3", dict(N=2, C=64, H=9, W=13, Cout=128, k=3, pad=1)),
                    ("c64-3x3-s2", dict(N=1, C=64, H=14, W=10, Cout=64, k=3, stride=2, pad=1)),
                    ("c32-3x3", dict(N=2, C=32, H=7, W=11, Cout=72, k=3, pad=1)),
                    ("c8-7x7-s2", dict(N=2, C=8, H=20, W=16, Cout=64, k=7, stride=2, pad=3)),
                    ("c128-1x1-s2-ntail", dict(N=2, C=128, H=10, W=6, Cout=200, k=1, stride=2)),
                    ("c16-4x4-outhw", dict(N=2, C=16, H=10, W=12, Cout=64, k=4, pad=2, out_hw=(10, 12))),
                    ("c64-2x2-outhw", dict(N=2, C=64, H=5, W=7, Cout=128, k=2, out_hw=(5, 7)))]:
        _both(cs, f"fast-conv-{cid}", "fast", _p("conv", relu=True, res=True, **kw), _pol(**off))

    # conv_pipe_kernel: conv and plain GEMM, one and two k-tiles, M = 81, the 256 x 256 form where Cout % 256 == 0
    pipe = dict(conv_stream=1, conv3x3_ws=1, skinny=1)
    for cid, kw, modes in [
            ("1x1-k64-m81", dict(N=1, C=64, H=9, W=9, Cout=256, k=1, res=True), (2, 3)),
            ("1x1-k128", dict(N=2, C=128, H=10, W=6, Cout=128, k=1, res=True, relu=True), (2,)),
            ("1x1-k64-ntail", dict(N=2, C=64, H=8, W=5, Cout=200, k=1, res=True, relu=True), (2,)),
            ("3x3", dict(N=1, C=64, H=9, W=7, Cout=64, k=3, pad=1), (2,)),
            ("3x3-s2", dict(N=1, C=128, H=12, W=8, Cout=256, k=3, stride=2, pad=1, relu=True), (2, 3))]:
        for mode in modes:
            _both(cs, f"pipe{mode}-conv-{cid}", "pipe", _p("conv", **kw), _pol(conv_pipe=mode, **pipe))
    for M, N, K, modes in [(300, 136, 192, (2,)), (300, 768, 320, (2, 3))]:
        for mode in modes:
            _both(cs, f"pipe{mode}-gemm-{M}x{N}x{K}", "pipe",
                  _p("gemm", M=M, N=N, K=K, cdt=BF, add1=BF, **nt), _pol(conv_pipe=mode, **pipe))

    _both(cs, "pipe2-gemm-plain-300x136x192", "pipe",
          _p("gemm", M=300, N=136, K=192, tA=False, tB=False, dtype=BF, cdt=BF), _pol(conv_pipe=2, **pipe))

    # conv1x1_stream_kernel: every K, both slice widths, M = 75 (a ragged last item), strided
    for K in (64, 128, 256, 512):
        for Cout in (128, 256):
            resid = (K // 64 + Cout // 128) % 2 == 1
            _both(cs, f"stream-k{K}-n{Cout}{'-res' if resid else ''}", "stream",
                  _p("conv", N=3, C=K, H=5, W=5, Cout=Cout, k=1, relu=resid, res=resid), _pol(conv_stream=2))
    _both(cs, "stream-strided", "stream", _p("conv", N=1, C=128, H=10, W=6, Cout=256, k=1, stride=2),
          _pol(conv_stream=2))
    _both(cs, "stream-strided-res", "stream",
          _p("conv", N=3, C=256, H=5, W=9, Cout=128, k=1, stride=2, relu=True, res=True), _pol(conv_stream=2))

    # conv1x1_chain_kernel / conv1x1_proj_kernel at the "ragged" shape (M = 75) of their own tests
    for K, N, N2 in [(64, 256, 64), (64, 256, 128), (128, 512, 128)]:
        _both(cs, f"chain-{K}-{N}-{N2}", "chain", _p("chain", K=K, N=N, N2=N2, B=3, H=5, W=5), _pol(conv_stream=2))
    for K, N, Kp, S, N2 in [(64, 256, 64, 1, 0), (64, 256, 64, 1, 64), (128, 512, 256, 2, 0)]:
        _both(cs, f"proj-{K}-{N}-{Kp}-s{S}-{N2}", "proj", _p("chain", K=K, N=N, N2=N2, Kp=Kp, S=S, B=3, H=5, W=5),
              _pol(conv_stream=2))

    # conv_ws_kernel (64 -> 64 3x3 at width 56 / 224, the 4x4 stem at width 112) and conv_stem_pool_kernel
    for cid, kw in [("w56", dict(N=2, C=64, H=8, W=56, Cout=64, k=3, pad=1, relu=True)),
                    ("w224", dict(N=1, C=64, H=4, W=224, Cout=64, k=3, pad=1, bias=False)),
                    ("stem", dict(N=2, C=16, H=6, W=112, Cout=64, k=4, pad=2, out_hw=(6, 112)))]:
        _both(cs, f"ws-{cid}", "ws", _p("conv", **kw))
    for N, H in [(1, 2), (3, 6)]:
        _both(cs, f"stempool-{N}x{H}", "stempool",
              _p("conv", N=N, C=16, H=H, W=112, Cout=64, k=4, pad=2, out_hw=(H, 112), relu=True, pool=(3, 2, 1)))

    # maxpool2d_nhwc
    for cid, kw in [("f32-3x3", dict(N=2, C=16, H=13, W=9, dtype=F32, pool=(3, 2, 1))),
                    ("f32-2x2", dict(N=2, C=16, H=14, W=10, dtype=F32, pool=(2, 2, 0))),
                    ("bf16-3x3", dict(N=2, C=64, H=12, W=20, dtype=BF, pool=(3, 2, 1))),
                    ("bf16-3x3-odd", dict(N=3, C=16, H=13, W=7, dtype=BF, pool=(3, 2, 1))),
                    ("bf16-2x2", dict(N=2, C=32, H=14, W=10, dtype=BF, pool=(2, 2, 0)))]:
        cs.append(Case(f"pool-{cid}", "pool", "exact", _p("pool", **kw), ()))

    # convblock.hip: every geometry the fragment kernels accept, N = 3 (and its first image alone)
    for H, C in [(14, 256), (14, 512), (28, 128), (7, 512), (112, 128), (56, 256)]:
        _both(cs, f"frag3x3-{H}x{H}x{C}", "frag3x3",
              _p("conv", N=3, C=C, H=H, W=H, Cout=C, k=3, pad=1, relu=True))
    _both(cs, "frag1x1", "frag1x1", _p("conv", N=3, C=1024, H=14, W=14, Cout=256, k=1, relu=True))
    for H, C, Cm in [(14, 1024, 256), (28, 512, 128)]:
        _both(cs, f"block-{H}x{H}x{C}", "block", _p("block", N=3, H=H, C=C, Cmid=Cm))

    # split_gemm_kernel: the smallest row of each operand form of its own test; (split_gemm, split_k) forms the
    # planner can honour at that K
    for M, N, K, tA, tB, beta, add1 in [(1000, 200, 1000, True, True, 0.0, None), (300, 136, 520, False, True, 1.0, None),
                                        (1024, 1024, 2048, True, False, 0.0, None), (300, 136, 1104, False, False, 0.0, F32),
                                        (3, 512, 2624, False, False, 1.0, None)]:
        p = _p("gemm", M=M, N=N, K=K, tA=tA, tB=tB, dtype=BF, cdt=F32, beta=beta, add1=add1)
        for form in (2, 3):
            for sk in ((2, 3) if K == 520 else (2, 4)):
                cs.append(Case(f"split{form}-k{sk}-{lay[(tA, tB)]}-{M}x{N}x{K}", "split", "small", p,
                               _pol(split_gemm=form, split_k=sk)))

    # skinny_gemm_kernel
    for M, N, K, bias in [(5, 96, 32, True), (33, 64, 96, False), (100, 128, 512, True), (128, 64, 1024, False)]:
        cs.append(Case(f"skinny-{M}x{N}x{K}", "skinny", "small",
                       _p("gemm", M=M, N=N, K=K, tA=False, tB=False, dtype=BF, cdt=F32, bias=bias), _pol(skinny=2)))

    # conv3x3_wgrad
    for N, H, W, Cin, Cout in [(3, 7, 7, 128, 128), (3, 5, 9, 256, 128), (2, 2, 2, 128, 128), (3, 7, 7, 128, 256)]:
        for dt in (BF, F32):
            for acc in (False, True):
                cs.append(Case(f"wgrad-{'bf16' if dt == BF else 'f32'}-{N}x{H}x{W}x{Cin}x{Cout}{'-acc' if acc else ''}",
                               "wgrad", "small", _p("wgrad", N=N, H=H, W=W, Cin=Cin, Cout=Cout, dtype=dt, accumulate=acc),
                               ()))
    # 288 tiles of 128 rows are more than one round of workgroups: the planner takes the 256-row tiles here
    cs.append(Case("wgrad-bf16-3x7x7x512x1024-rows256", "wgrad", "small",
                   _p("wgrad", N=3, H=7, W=7, Cin=512, Cout=1024, dtype=BF, accumulate=True), ()))
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _table()
FAMILIES = sorted({c.family for c in CASES})

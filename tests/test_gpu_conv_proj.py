"""The projection forms of the 1x1 stream kernel (csrc/convstream.hip, sat_conv1x1_proj): the c3 of a stage's first
bottleneck with the downsample conv of the block input formed in registers as its residual, plain and chained into
the next block's c1 -- against the separate launches (bit for bit) and an fp32 CPU product -- and the Encoder
attributes that use them (``proj_l1``, ``proj_l2``).  Every test here needs an MI355X.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (K, N, Kp, stride, N2 (0: plain), rows per item): layer1 block 0 plain / chained into block 1, layer2 block 0
FORMS = [(64, 256, 64, 1, 0, 64), (64, 256, 64, 1, 64, 64), (128, 512, 256, 2, 0, 32)]


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


def rel(a, b):
    a = a.double().cpu(); b = b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def close(out, ref):
    """test_gpu_conv_chain's bound (bf16 output of an fp32 sum over exact bf16 operands)."""
    out, ref = out.float().cpu(), ref.float().cpu()
    return rel(out, ref) < 1e-2 and bool(((out - ref).abs() <= 1e-2 * ref.abs() + 2e-2).all())


def folded(cout, cin, g, dtype=torch.bfloat16, stride=1):
    """(w [Cout,1,1,Cin], bias f32, stride, pad) as the Encoder plan holds a folded 1x1 conv."""
    w = (torch.randn(cout, 1, 1, cin, generator=g) / math.sqrt(cin)).to(dtype)
    return (w.to(DEV), torch.randn(cout, generator=g).to(DEV), stride, 0)


def shapes(which, mt):
    """test_gpu_conv_chain's three kinds, as the c3's (B, OH, OW)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"ragged": (3, 5, 5),              # M = 75: a ragged last item at 32- and 64-row items
            "few": (1, 56, 56),               # M = 3136: fewer items than workgroups, idle ones return early
            "wrap": (1, 4 * cus + 3, mt)}[which]   # >= 4 items per workgroup: the ring wraps, some run one more


def separate(ops, x, c3, xin, ds, c1n, pol):
    """The launches the projection kernel stands for."""
    idn = ops.conv2d_nhwc(xin, *ds, False, policy=pol)
    y = ops.conv2d_nhwc(x, *c3, True, residual=idn, policy=pol)
    return idn, y, (ops.conv2d_nhwc(y, *c1n, True, policy=pol) if c1n is not None else None)


@pytest.mark.parametrize("which", ["ragged", "few", "wrap"])
@pytest.mark.parametrize("K,N,KP,S,N2,MT", FORMS)
def test_proj_kernel(sat, K, N, KP, S, N2, MT, which):
    from sat_amd import ops
    B, H, W = shapes(which, MT)
    g = torch.Generator().manual_seed(K + N + KP + N2 + B * H * W)
    force, off = sat.Policy(conv_stream=2), sat.Policy(conv_stream=1)
    c3, ds = folded(N, K, g), folded(N, KP, g, stride=S)
    c1n = folded(N2, N, g) if N2 else None
    x = torch.randn(B, H, W, K, generator=g).bfloat16().to(DEV)
    xin = torch.randn(B, S * H, S * W, KP, generator=g).bfloat16().to(DEV)   # stride 2: the block input is 2H x 2W
    assert ops.conv1x1_proj_supported(B * H * W, K, N, KP, S, N2, torch.bfloat16, force)
    proj = ops.ProjectedResidual(xin, ds)
    if N2:
        y, x1 = ops.conv1x1_chain(x, c3, proj, c1n, policy=force)
    else:
        y, x1 = ops.conv2d_nhwc(x, *c3, True, residual=proj, policy=force), None
    for pol in (force, off):   # the separate launches on the stream kernel where eligible, then never
        idn, y2, x2 = separate(ops, x, c3, xin, ds, c1n, pol)
        assert torch.equal(y, y2)
        if N2:
            assert torch.equal(x1, x2)
    xs = xin[:, ::S, ::S, :].float().cpu().reshape(-1, KP)
    idr = (xs @ ds[0].float().cpu().reshape(N, KP).T + ds[1].cpu()).bfloat16().float()
    yr = torch.relu(x.float().cpu().reshape(-1, K) @ c3[0].float().cpu().reshape(N, K).T + c3[1].cpu() + idr)
    assert close(y.reshape(-1, N), yr)
    if N2:
        xr = torch.relu(y.float().cpu().reshape(-1, N) @ c1n[0].float().cpu().reshape(N2, N).T + c1n[1].cpu())
        assert close(x1.reshape(-1, N2), xr)


@pytest.mark.parametrize("K,N,KP,S,N2,MT", FORMS)
def test_proj_auto_threshold(sat, K, N, KP, S, N2, MT):
    """Auto mode takes what the c3's own stream / chained launch takes; conv_stream=1 nothing; other shapes never."""
    from sat_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bf = torch.bfloat16
    slices = 1 if N2 else N // 256
    M = 2 * cus * MT // slices
    assert ops.conv1x1_proj_supported(M, K, N, KP, S, N2, bf)
    assert not ops.conv1x1_proj_supported(M - MT, K, N, KP, S, N2, bf)
    assert not ops.conv1x1_proj_supported(M, K, N, KP, S, N2, bf, sat.Policy(conv_stream=1))
    assert not ops.conv1x1_proj_supported(M, K, N, KP, S, N2, torch.float32, sat.Policy(conv_stream=2))
    assert not ops.conv1x1_proj_supported(M, K, N, KP, 3 - S, N2, bf, sat.Policy(conv_stream=2))
    assert not ops.conv1x1_proj_supported(M, K, N, 2 * KP, S, N2, bf, sat.Policy(conv_stream=2))
    assert not ops.conv1x1_proj_supported(M, K, N, KP, S, 128, bf, sat.Policy(conv_stream=2))
    assert not ops.conv1x1_proj_supported((1 << 31) // N, K, N, KP, S, N2, bf, sat.Policy(conv_stream=2))


@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("dtype,mode,M", [(torch.float32, 2, 75), (torch.bfloat16, 0, 75), (torch.bfloat16, 1, 75)])
def test_proj_fallback(sat, dtype, mode, M, chained):
    """Where the projection kernel does not run (fp32, below the auto threshold, conv_stream=1) the call issues the
    downsample launch and then today's launches: same bits."""
    from sat_amd import ops
    K, N, KP, N2 = 64, 256, 64, 64 if chained else 0
    g = torch.Generator().manual_seed(13)
    pol = sat.Policy(conv_stream=mode)
    assert not ops.conv1x1_proj_supported(M, K, N, KP, 1, N2, dtype, pol)
    c3, ds = folded(N, K, g, dtype), folded(N, KP, g, dtype)
    c1n = folded(N2, N, g, dtype) if chained else None
    x = torch.randn(3, 5, 5, K, generator=g).to(dtype).to(DEV)
    xin = torch.randn(3, 5, 5, KP, generator=g).to(dtype).to(DEV)
    proj = ops.ProjectedResidual(xin, ds)
    if chained:
        y, x1 = ops.conv1x1_chain(x, c3, proj, c1n, policy=pol)
    else:
        y, x1 = ops.conv2d_nhwc(x, *c3, True, residual=proj, policy=pol), None
    _, y2, x2 = separate(ops, x, c3, xin, ds, c1n, pol)
    assert torch.equal(y, y2) and (not chained or torch.equal(x1, x2))


# ---------------------------------------------------------------------------- Encoder
@pytest.fixture(scope="module")
def trunk(sat):
    """bf16 ResNet152, B = 2 at 224 x 224, every eligible 1x1 forced onto the stream kernels (B = 2 is below the
    auto threshold), and its features with both projection attributes off -- the reference, computed once."""
    torch.manual_seed(5)
    enc = sat.Encoder("resnet152", dtype=torch.bfloat16).to(DEV).eval()
    enc.policy = sat.Policy(conv_stream=2)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(9)).to(DEV)
    enc.proj_l1 = enc.proj_l2 = False
    with torch.no_grad():
        ref = enc(x).clone()
    enc.proj_l1 = enc.proj_l2 = True
    return enc, x, ref


def run(enc, x, on, chain={64}, split=False):
    enc.proj_l1 = enc.proj_l2 = on
    enc.chain_c1 = chain
    try:
        with torch.no_grad():
            if not split:
                return enc(x)
            n = len(enc.compiled_plan(x.device, torch.bfloat16))
            cuts = [0] + enc.stage_starts() + [n]
            y = x
            for a, b in zip(cuts, cuts[1:]):
                y = enc(y, steps=(a, b))
            return y
    finally:
        enc.proj_l1 = enc.proj_l2 = True
        enc.chain_c1 = {64}


def count_proj(monkeypatch):
    from sat_amd import ops
    calls = []
    real = ops._proj_launch

    def counted(x, c3, proj, c1_next, policy):
        r = real(x, c3, proj, c1_next, policy)
        calls.append((x.shape[3], c1_next[0].shape[0] if c1_next is not None else 0, r is not None))
        return r
    monkeypatch.setattr(ops, "_proj_launch", counted)
    return calls


def test_encoder_default_on(sat):
    enc = sat.Encoder("vgg19")
    assert enc.proj_l1 is True and enc.proj_l2 is True


@pytest.mark.parametrize("chain,forms", [({64}, [(64, 64, True), (128, 0, True)]),
                                         (set(), [(64, 0, True), (128, 0, True)]),
                                         ({64, 128}, [(64, 64, True)])])
def test_encoder_proj_bits(sat, trunk, monkeypatch, chain, forms):
    """Attributes on = attributes off, bit for bit; layer1 takes the chained or the plain form with chain_c1, and
    layer2's chained c3 declines the projection (it keeps its downsample launch)."""
    enc, x, ref = trunk
    calls = count_proj(monkeypatch)
    assert torch.equal(run(enc, x, True, chain), ref)
    assert sorted(calls) == sorted(forms)
    assert torch.equal(run(enc, x, False, chain), ref)
    assert len(calls) == len(forms)


def test_encoder_proj_steps_split(sat, trunk, monkeypatch):
    """The forward cut at stage_starts(): a slice that starts at a stage's first block projects from its own input."""
    enc, x, ref = trunk
    calls = count_proj(monkeypatch)
    assert torch.equal(run(enc, x, True, split=True), ref)
    assert sorted(calls) == [(64, 64, True), (128, 0, True)]


def test_encoder_proj_hook_records(sat, trunk):
    """The bench hooks see the same records (count, order, shapes), event pairs and launch-policy slots with the
    attributes on and off: an absorbed downsample launch keeps its record after c2 and before c3."""
    enc, x, ref = trunk
    recs = {}
    for on in (False, True):
        slots = []

        def next_policy():
            slots.append(1)
            return enc.policy
        enc.timing, enc.timing_args, enc.launch_policy = [], [], next_policy
        try:
            y = run(enc, x, on)
            recs[on] = (enc.timing_args, len(enc.timing), len(slots))
        finally:
            enc.timing = enc.timing_args = enc.launch_policy = None
        assert torch.equal(y, ref)
    (a0, t0, s0), (a1, t1, s1) = recs[False], recs[True]
    assert len(a0) == len(a1) == t0 == t1 == s0 == s1

    def shape_of(r):   # conv records: (x, w, ...); fragment-weight records: (kind, x, ...)
        return (r[0],) if isinstance(r[0], str) else (tuple(r[0].shape), tuple(r[1].shape))
    assert [shape_of(r) for r in a0] == [shape_of(r) for r in a1]


def test_encoder_proj_off_paths(sat, trunk, monkeypatch):
    """conv_stream=1 and an fp32 trunk: no projection kernel runs and the features are what they were."""
    enc, x, ref = trunk
    calls = count_proj(monkeypatch)
    enc.policy = sat.Policy(conv_stream=1)
    try:
        assert torch.equal(run(enc, x, True), ref)
    finally:
        enc.policy = sat.Policy(conv_stream=2)
    e32 = sat.Encoder("resnet152", dtype=torch.float32).to(DEV).eval()
    xs = x[:1, :, :64, :64].contiguous()
    assert torch.equal(run(e32, xs, True), run(e32, xs, False))
    assert calls == []

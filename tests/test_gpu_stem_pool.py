"""ResNet152's stem conv + ReLU + 3x3 / stride 2 / pad 1 max pool as one launch (csrc/conv3x3ws.hip,
sat_conv_stem_pool) against the two launches (bit for bit) and an fp32 CPU reference, and the Encoder with its three
trunk-entry attributes (``stem_pool``, ``proj_l1``, ``proj_l2``) on against all off.  Every test here needs an MI355X.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
POOL = (3, 2, 1)
W112 = 112   # the stem's width over the space-to-depth input of a 224-wide image


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


def stem(g, dtype=torch.bfloat16, bias_shift=0.0):
    """Random folded stem weights [64, 4, 4, 16] (the 4x4 / stride 1 / pad 2 form over s2d16) and biases."""
    w = (torch.randn(64, 4, 4, 16, generator=g) / math.sqrt(256)).to(dtype)
    return w.to(DEV), (torch.randn(64, generator=g) + bias_shift).to(DEV)


def two_launches(ops, x, w, b, policy=None):
    y = ops.conv2d_nhwc(x, w, b, 1, 2, True, out_hw=(x.shape[1], x.shape[2]), policy=policy)
    return ops.maxpool2d_nhwc(y, *POOL)


# N, H (conv rows), bias shift: one item with both image edges; images smaller than a run and fewer items than
# workgroups; run boundaries inside an image (the recomputed row above a run); 2072 items, some workgroups with two
# runs, the ring wraps; whole windows zero after ReLU
CASES = [(1, 2, 0.0), (3, 6, 0.0), (2, 112, 0.0), (37, 112, 0.0), (2, 6, -50.0), (2, 112, -3.0)]


@pytest.mark.parametrize("N,H,shift", CASES)
def test_stem_pool_kernel(sat, N, H, shift):
    from sat_amd import ops
    g = torch.Generator().manual_seed(N * 1000 + H)
    w, b = stem(g, bias_shift=shift)
    x = torch.randn(N, H, W112, 16, generator=g).bfloat16().to(DEV)
    assert ops.conv_stem_pool_supported(x, w, 1, 2, True, POOL, (H, W112))
    y = ops.conv_stem_pool(x, w, b, 1, 2, True, POOL, out_hw=(H, W112))
    assert y.shape == (N, H // 2, W112 // 2, 64)
    assert torch.equal(y, two_launches(ops, x, w, b))
    assert torch.equal(y, two_launches(ops, x, w, b, sat.Policy(conv3x3_ws=1)))   # the tile kernel's conv
    if shift <= -50.0:
        assert not y.any()
    if N <= 3:   # fp32 on the same bf16 operands: bottom / right padding 1 gives the conv H x 112 outputs
        xc = torch.nn.functional.pad(x.float().cpu().permute(0, 3, 1, 2), (2, 1, 2, 1))
        c = torch.nn.functional.conv2d(xc, w.float().cpu().permute(0, 3, 1, 2), b.cpu())
        ref = torch.nn.functional.max_pool2d(torch.relu(c).bfloat16().float(), *POOL).permute(0, 2, 3, 1)
        assert close(y, ref)


def test_stem_pool_fallback(sat):
    """fp32, an odd height, another width, no ReLU, another pool, the weight-stationary kernel off: not supported,
    and the call issues conv then pool -- the same bits."""
    from sat_amd import ops
    g = torch.Generator().manual_seed(21)
    for dtype, H, W, relu, pool, pol in [(torch.float32, 6, W112, True, POOL, None),
                                         (torch.bfloat16, 5, W112, True, POOL, None),
                                         (torch.bfloat16, 6, 56, True, POOL, None),
                                         (torch.bfloat16, 6, W112, False, POOL, None),
                                         (torch.bfloat16, 6, W112, True, (2, 2, 0), None),
                                         (torch.bfloat16, 6, W112, True, POOL, sat.Policy(conv3x3_ws=1))]:
        w, b = stem(g, dtype)
        x = torch.randn(2, H, W, 16, generator=g).to(dtype).to(DEV)
        assert not ops.conv_stem_pool_supported(x, w, 1, 2, relu, pool, (H, W), pol)
        y = ops.conv_stem_pool(x, w, b, 1, 2, relu, pool, out_hw=(H, W), policy=pol)
        y2 = ops.maxpool2d_nhwc(ops.conv2d_nhwc(x, w, b, 1, 2, relu, out_hw=(H, W), policy=pol), *pool)
        assert torch.equal(y, y2)


# ---------------------------------------------------------------------------- Encoder: the three attributes together
def set_entry(enc, on):
    enc.stem_pool = enc.proj_l1 = enc.proj_l2 = on


@pytest.fixture(scope="module")
def trunk(sat):
    """bf16 ResNet152, B = 2 at 224 x 224, every eligible 1x1 forced onto the stream kernels (B = 2 is below the
    auto threshold), and its features with the three attributes off -- the reference, computed once."""
    torch.manual_seed(4)
    enc = sat.Encoder("resnet152", dtype=torch.bfloat16).to(DEV).eval()
    enc.policy = sat.Policy(conv_stream=2)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(10)).to(DEV)
    set_entry(enc, False)
    with torch.no_grad():
        ref = enc(x).clone()
    set_entry(enc, True)
    return enc, x, ref


def run(enc, x, on, split=False):
    set_entry(enc, on)
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
        set_entry(enc, True)


def count(monkeypatch, name):
    from sat_amd import ops
    calls = []
    real = getattr(ops, name)

    def counted(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return calls


def test_encoder_default_on(sat):
    enc = sat.Encoder("vgg19")
    assert enc.stem_pool is True and enc.proj_l1 is True and enc.proj_l2 is True


def test_encoder_entry_bits(sat, trunk, monkeypatch):
    enc, x, ref = trunk
    fused, pools = count(monkeypatch, "conv_stem_pool"), count(monkeypatch, "maxpool2d_nhwc")
    assert torch.equal(run(enc, x, True), ref)
    assert (len(fused), len(pools)) == (1, 0)
    assert torch.equal(run(enc, x, False), ref)
    assert (len(fused), len(pools)) == (1, 1)


def test_encoder_entry_packed_images(sat, trunk, monkeypatch):
    """The packed-image entry path takes the fused stem too."""
    from sat_amd.data import PackedImages
    enc, _, _ = trunk
    g = torch.Generator().manual_seed(12)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in ((224, 224), (240, 250))]
    packed = PackedImages.from_arrays(imgs).to(DEV)
    fused = count(monkeypatch, "conv_stem_pool")
    on = run(enc, packed, True)
    assert len(fused) == 1
    assert torch.equal(on, run(enc, packed, False))


def test_encoder_entry_steps_split(sat, trunk, monkeypatch):
    """The forward cut at stage_starts(): stem and pool share the first slice."""
    enc, x, ref = trunk
    fused = count(monkeypatch, "conv_stem_pool")
    assert torch.equal(run(enc, x, True, split=True), ref)
    assert len(fused) == 1


def test_encoder_entry_pool_outside_slice(sat, trunk, monkeypatch):
    """A slice that ends between the stem and the pool runs the conv alone."""
    enc, x, ref = trunk
    fused = count(monkeypatch, "conv_stem_pool")
    n = len(enc.compiled_plan(x.device, torch.bfloat16))
    with torch.no_grad():
        y = enc(x, steps=(0, 1))
        assert y.shape[1:] == (112, 112, 64)
        y = enc(y, steps=(1, n))
    assert fused == [] and torch.equal(y, ref)


def test_encoder_entry_hook_records(sat, trunk):
    """The bench hooks see the same records (count, order, shapes), event pairs and launch-policy slots with the
    attributes on and off: the stem keeps its one record, an absorbed downsample launch its place."""
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

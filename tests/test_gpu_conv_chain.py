"""The chained 1x1 kernel (csrc/convstream.hip, sat_conv1x1_chain): a bottleneck's c3 + residual + ReLU and the
next bottleneck's c1 + ReLU in one launch, against the two separate launches (bit for bit) and torch fp32, and
the Encoder hand-off that uses it.  Every test here needs an MI355X.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (K, N, N2, rows per item): layer1 block -> block, layer1 -> layer2, layer2 block -> block
INSTANCES = [(64, 256, 64, 64), (64, 256, 128, 64), (128, 512, 128, 32)]


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
    """test_conv_stream_kernel's bound (bf16 output of an fp32 sum over exact bf16 operands)."""
    out, ref = out.float().cpu(), ref.float().cpu()
    return rel(out, ref) < 1e-2 and bool(((out - ref).abs() <= 1e-2 * ref.abs() + 2e-2).all())


def folded(cout, cin, g, dtype=torch.bfloat16):
    """(w [Cout,1,1,Cin], bias f32, stride, pad) as the Encoder plan holds a folded 1x1 conv."""
    w = (torch.randn(cout, 1, 1, cin, generator=g) / math.sqrt(cin)).to(dtype)
    return (w.to(DEV), torch.randn(cout, generator=g).to(DEV), 1, 0)


def shapes(which, mt):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"ragged": (3, 5, 5),              # M = 75: a ragged last item at 32- and 64-row items
            "few": (1, 56, 56),               # M = 3136: fewer items than workgroups, idle ones return early
            "wrap": (1, 4 * cus + 3, mt)}[which]   # >= 4 items per workgroup: the ring wraps, 3 workgroups run one more


@pytest.mark.parametrize("resid", ["identity", "separate"])
@pytest.mark.parametrize("which", ["ragged", "few", "wrap"])
@pytest.mark.parametrize("K,N,N2,MT", INSTANCES)
def test_chain_kernel(sat, K, N, N2, MT, which, resid):
    from sat_amd import ops
    B, H, W = shapes(which, MT)
    g = torch.Generator().manual_seed(K + N + N2 + B * H * W)
    force, off = sat.Policy(conv_stream=2), sat.Policy(conv_stream=1)
    c3, c1n = folded(N, K, g), folded(N2, N, g)
    if resid == "identity":   # the block's own input: x comes from it, as in an identity bottleneck
        res = torch.randn(B, H, W, N, generator=g).bfloat16().to(DEV)
        x = ops.conv2d_nhwc(res, *folded(K, N, g), True)
    else:
        res = torch.randn(B, H, W, N, generator=g).bfloat16().to(DEV)
        x = torch.randn(B, H, W, K, generator=g).bfloat16().to(DEV)
    assert ops.conv1x1_chain_supported(B * H * W, K, N, N2, torch.bfloat16, force)
    y, x1 = ops.conv1x1_chain(x, c3, res, c1n, policy=force)
    for pol in (force, off):   # the separate launches on the stream kernel where eligible, then never
        y2 = ops.conv2d_nhwc(x, *c3, True, residual=res, policy=pol)
        x2 = ops.conv2d_nhwc(y2, *c1n, True, policy=pol)
        assert torch.equal(y, y2) and torch.equal(x1, x2)
    yr = torch.relu(x.float().cpu().reshape(-1, K) @ c3[0].float().cpu().reshape(N, K).T + c3[1].cpu()
                    + res.float().cpu().reshape(-1, N))
    assert close(y.reshape(-1, N), yr)
    xr = torch.relu(y.float().cpu().reshape(-1, N) @ c1n[0].float().cpu().reshape(N2, N).T + c1n[1].cpu())
    assert close(x1.reshape(-1, N2), xr)


@pytest.mark.parametrize("K,N,N2,MT", INSTANCES)
def test_chain_auto_threshold(sat, K, N, N2, MT):
    """Auto mode takes problems of at least 2 x CUs items, conv_stream=1 none, other shapes never."""
    from sat_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bf = torch.bfloat16
    assert ops.conv1x1_chain_supported(2 * cus * MT, K, N, N2, bf)
    assert not ops.conv1x1_chain_supported(2 * cus * MT - MT, K, N, N2, bf)
    assert not ops.conv1x1_chain_supported(2 * cus * MT, K, N, N2, bf, sat.Policy(conv_stream=1))
    assert not ops.conv1x1_chain_supported(2 * cus * MT, K, N, N2, torch.float32, sat.Policy(conv_stream=2))
    assert not ops.conv1x1_chain_supported(2 * cus * MT, K, N, 2 * N2 + 64, bf, sat.Policy(conv_stream=2))
    assert not ops.conv1x1_chain_supported((1 << 31) // N, K, N, N2, bf, sat.Policy(conv_stream=2))


@pytest.mark.parametrize("dtype,mode", [(torch.bfloat16, 1), (torch.float32, 2)])
def test_chain_fallback(sat, dtype, mode):
    """Where the chained kernel does not run (conv_stream=1, fp32) the call issues the two launches: same bits."""
    from sat_amd import ops
    K, N, N2 = 64, 256, 64
    g = torch.Generator().manual_seed(11)
    pol = sat.Policy(conv_stream=mode)
    assert not ops.conv1x1_chain_supported(75, K, N, N2, dtype, pol)
    c3, c1n = folded(N, K, g, dtype), folded(N2, N, g, dtype)
    x = torch.randn(3, 5, 5, K, generator=g).to(dtype).to(DEV)
    res = torch.randn(3, 5, 5, N, generator=g).to(dtype).to(DEV)
    y, x1 = ops.conv1x1_chain(x, c3, res, c1n, policy=pol)
    y2 = ops.conv2d_nhwc(x, *c3, True, residual=res, policy=pol)
    x2 = ops.conv2d_nhwc(y2, *c1n, True, policy=pol)
    assert torch.equal(y, y2) and torch.equal(x1, x2)


# ---------------------------------------------------------------------------- Encoder hand-off
@pytest.fixture(scope="module")
def trunk(sat):
    """bf16 ResNet152, B = 2 at 224 x 224, every eligible 1x1 forced onto the stream kernels (B = 2 is below the
    auto threshold), and its features with every c1 its own launch -- the reference, computed once."""
    torch.manual_seed(3)
    enc = sat.Encoder("resnet152", dtype=torch.bfloat16).to(DEV).eval()
    enc.policy = sat.Policy(conv_stream=2)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(8)).to(DEV)
    ref = {}
    enc.chain_c1 = set()
    with torch.no_grad():
        for f2 in (False, True):
            enc.fuse_layer2 = f2
            ref[f2] = enc(x).clone()
    enc.fuse_layer2 = False
    return enc, x, ref


def run(enc, x, chain, fuse2=False, split=False):
    enc.chain_c1, enc.fuse_layer2 = chain, fuse2
    try:
        with torch.no_grad():
            if not split:
                return enc(x)
            n = len(enc.compiled_plan(x.device, torch.bfloat16))
            cuts = [0] + enc.stage_starts()[1:] + [n]
            y = x
            for a, b in zip(cuts, cuts[1:]):
                y = enc(y, steps=(a, b))
            return y
    finally:
        enc.chain_c1, enc.fuse_layer2 = {64}, False


def count_chained(enc, monkeypatch):
    from sat_amd import ops
    calls = []
    real = ops.conv1x1_chain

    def counted(x, c3, residual, c1_next, policy=None):
        calls.append((x.shape[3], c1_next[0].shape[0]))
        return real(x, c3, residual, c1_next, policy=policy)
    monkeypatch.setattr(ops, "conv1x1_chain", counted)
    return calls


def test_encoder_default_chains(sat):
    """Layer1's chains are on by default; layer2's are built and tested but off."""
    assert sat.Encoder("vgg19").chain_c1 == {64}


@pytest.mark.parametrize("chain,n", [({64, 128}, 10), ({64}, 3), ({128}, 7)])
def test_encoder_chain_bits(sat, trunk, monkeypatch, chain, n):
    enc, x, ref = trunk
    calls = count_chained(enc, monkeypatch)
    assert torch.equal(run(enc, x, chain), ref[False])
    assert len(calls) == n and all(k in chain for k, _ in calls)


def test_encoder_chain_steps_split(sat, trunk, monkeypatch):
    """Slices at stage_starts(): the hand-off never crosses a slice, so layer1 -> layer2 is not chained."""
    enc, x, ref = trunk
    calls = count_chained(enc, monkeypatch)
    assert torch.equal(run(enc, x, {64, 128}, split=True), ref[False])
    assert sorted(calls) == [(64, 64)] * 2 + [(128, 128)] * 7


def test_encoder_chain_fuse_layer2(sat, trunk, monkeypatch):
    """Blocks that run fused are never chained into: layer1's chains and layer2's first c1 remain."""
    enc, x, ref = trunk
    calls = count_chained(enc, monkeypatch)
    assert torch.equal(run(enc, x, {64, 128}, fuse2=True), ref[True])
    assert sorted(calls) == [(64, 64)] * 2 + [(64, 128)]


def test_encoder_chain_hook_records(sat, trunk, monkeypatch):
    """The bench hooks see one record, one event pair and one launch-policy slot per conv launch of the unchained
    forward, in the same order; the 10 absorbed c1 launches keep theirs."""
    enc, x, ref = trunk
    recs = {}
    for chain in (set(), {64, 128}):
        slots = []

        def next_policy():
            slots.append(1)
            return enc.policy
        enc.timing, enc.timing_args, enc.launch_policy = [], [], next_policy
        calls = count_chained(enc, monkeypatch) if chain else []
        try:
            y = run(enc, x, chain)
            recs[bool(chain)] = (enc.timing_args, len(enc.timing), len(slots), len(calls))
        finally:
            enc.timing = enc.timing_args = enc.launch_policy = None
        assert torch.equal(y, ref[False])
    (a0, t0, s0, c0), (a1, t1, s1, c1) = recs[False], recs[True]
    assert len(a0) == len(a1) == t0 == t1 == s0 == s1 and (c0, c1) == (0, 10)

    def shape_of(r):   # conv records: (x, w, ...); fragment-weight records: (kind, x, ...)
        return (r[0],) if isinstance(r[0], str) else (tuple(r[0].shape), tuple(r[1].shape))
    assert [shape_of(r) for r in a0] == [shape_of(r) for r in a1]


def test_encoder_chain_off_paths(sat, trunk):
    """conv_stream=1 and an fp32 trunk: nothing is chained and the features are what they were."""
    enc, x, ref = trunk
    enc.policy = sat.Policy(conv_stream=1)
    try:
        assert torch.equal(run(enc, x, {64, 128}), run(enc, x, set()))
        assert torch.equal(run(enc, x, {64, 128}), ref[False])
    finally:
        enc.policy = sat.Policy(conv_stream=2)
    e32 = sat.Encoder("resnet152", dtype=torch.float32).to(DEV).eval()
    xs = x[:1, :, :64, :64].contiguous()
    assert torch.equal(run(e32, xs, {64, 128}), run(e32, xs, set()))

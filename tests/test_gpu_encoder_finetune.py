"""conv3x3_wgrad_kernel (csrc/convwgrad.hip, sat_conv3x3_wgrad): the weight gradient of a 3x3 / stride-1 / pad-1
convolution on NHWC bf16 tensors -- autograd's conv.weight gradient for the c2 of a torchvision Bottleneck
(encoder.py:13-17) and VGG19's block-5 convolutions (encoder.py:24-27), the hot-path kernel of fine-tuning the top of
the encoder.

Every shape runs with the planner's split count and with forced ones (SatPolicy.split_k = 1, 2, 3; 3 splits the
k-tiles raggedly), against an fp64 product of the same bf16 operands.  The bound per element is the first-order
bound of a K-term fp32 accumulation of exact bf16 products, |error| <= 2 K 2^-24 sum |dz| |x| (a product of two
bf16 values is exact in fp32; K additions each round by at most 2^-24 relative; the factor 2 covers the split sums
and second-order terms).  X = 1, dZ = 1 counts the pixels under each tap and must be exact; accumulation adds the
fp32 product onto the prior buffer in one fp32 addition, so it is compared bit for bit; and the fixed summation order
makes repeated calls bit-identical.  Guard words around the output catch a store outside it.

The second half covers the trainable tail built on it (Encoder.fine_tune): sat_conv_fold against
Encoder._fold, the unit backwards in fp32 against fp64 autograd over the oracle's blocks and in bf16 against an fp64
mirror that rounds where the HIP path rounds, a train step through the decoder with the partial plan refresh, graph
capture, and fine_tune = 0 against the frozen encoder.  The tail is fed a random NHWC activation at plan step
tail_start(), so the frozen convs are not run.  Measured (MI355X): fp32 worst 1.7e-6 of the norm / 2.1e-6 of max |g|;
bf16 worst 5.1e-4 (ResNet152 n = 2), 1.1e-3 (VGG19 n = 4), 1.1e-7 (ResNet152 n = 1 at 2x2).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, H, W, Cin, Cout)
SHAPES = [
    (3, 7, 7, 128, 128),     # K = 147: two k-tiles plus a tail, image boundaries inside a k-tile
    (2, 14, 14, 128, 128),   # the 14 x 14 spatial size
    (3, 5, 9, 256, 128),     # non-square image, Cin != Cout: row / column and transposition mistakes
    (2, 2, 2, 128, 128),     # almost every tap is padding
    (6, 7, 7, 512, 512),     # the production channel count: 144 output tiles
]
SPLITS = [0, 1, 2, 3]
# the planner's own choice at a long K: 256-row tiles and three splits (72 x 3 workgroups, 25 k-tiles)
LONG_K = (32, 7, 7, 512, 512)
GUARD = 32   # fp32 words before and after the output


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


def _im2col(x):
    """x [N,H,W,C] -> [N H W, 9 C], column (kh 3 + kw) C + c = x[n, oh + kh - 1, ow + kw - 1, c] (zero outside)."""
    N, H, W, C = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    cols = [xp[:, kh:kh + H, kw:kw + W, :] for kh in range(3) for kw in range(3)]
    return torch.stack(cols, dim=3).reshape(N * H * W, 9 * C)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """bf16 operands on the device, the fp64 gradient and the element bound (computed once per shape)."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + Cin + 3 * Cout)
    x = torch.randn(N, H, W, Cin, generator=g).bfloat16().to(DEV)
    dz = torch.randn(N, H, W, Cout, generator=g).bfloat16().to(DEV)
    prior = torch.randn(Cout, 3, 3, Cin, generator=g).to(DEV)
    cols = _im2col(x.double())
    dz2 = dz.double().reshape(-1, Cout)
    ref = (dz2.T @ cols).reshape(Cout, 3, 3, Cin)
    mag = (dz2.abs().T @ cols.abs()).reshape(Cout, 3, 3, Cin)
    K = N * H * W
    return x, dz, prior, ref, 2.0 * K * 2.0 ** -24 * mag


def _run(sat, x, dz, split_k, prior=None):
    """One call into a guarded buffer -> (dw, guards intact)."""
    from sat_amd import ops
    Cout, Cin = dz.shape[3], x.shape[3]
    n = Cout * 9 * Cin
    flat = torch.full((n + 2 * GUARD,), 7.0, device=DEV)
    out = flat[GUARD:GUARD + n].view(Cout, 3, 3, Cin)
    if prior is not None:
        out.copy_(prior)
    else:
        out.fill_(float("nan"))   # beta = 0 never reads the buffer
    ops.conv3x3_wgrad(x, dz, out=out, accumulate=prior is not None, policy=sat.Policy(split_k=split_k))
    torch.cuda.synchronize()
    return out.clone(), bool((flat[:GUARD] == 7.0).all() and (flat[GUARD + n:] == 7.0).all())


@pytest.mark.parametrize("shape", SHAPES + [LONG_K], ids=lambda s: "x".join(map(str, s)))
def test_wgrad_matches_fp64(sat, shape):
    x, dz, prior, ref, bound = _case(shape)
    for s in SPLITS if shape != LONG_K else [0, 2]:
        dw, guards = _run(sat, x, dz, s)
        assert guards, s
        assert torch.isfinite(dw).all(), s
        err = (dw.double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{shape} split_k={s}: max |error| / bound = {worst:.3f}")
        assert (err <= bound).all(), (s, worst)


@pytest.mark.parametrize("shape", SHAPES + [LONG_K], ids=lambda s: "x".join(map(str, s)))
def test_wgrad_accumulates_and_repeats_bit_for_bit(sat, shape):
    x, dz, prior, ref, bound = _case(shape)
    for s in SPLITS if shape != LONG_K else [0, 2]:
        dw, _ = _run(sat, x, dz, s)
        again, _ = _run(sat, x, dz, s)
        assert torch.equal(dw, again), s
        acc, guards = _run(sat, x, dz, s, prior=prior)
        assert guards, s
        assert torch.equal(acc, dw + prior), s   # one fp32 addition of the product onto the prior buffer


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_of_ones_counts_pixels_exactly(sat, shape):
    N, H, W, Cin, Cout = shape
    x = torch.ones(N, H, W, Cin, dtype=torch.bfloat16, device=DEV)
    dz = torch.ones(N, H, W, Cout, dtype=torch.bfloat16, device=DEV)
    want = torch.tensor([[N * (H - abs(kh - 1)) * (W - abs(kw - 1)) for kw in range(3)] for kh in range(3)],
                        dtype=torch.float32, device=DEV)[None, :, :, None].expand(Cout, 3, 3, Cin)
    for s in SPLITS:
        dw, guards = _run(sat, x, dz, s)
        assert guards, s
        assert torch.equal(dw, want), s


def test_wgrad_without_workspace_runs_unsplit(sat):
    from sat_amd import ops
    x, dz, prior, ref, bound = _case(SHAPES[0])
    dw = ops.conv3x3_wgrad(x, dz, workspace=None)
    one, _ = _run(sat, x, dz, 1)
    assert torch.equal(dw, one)


def test_wgrad_fp32_parity_path(sat):
    """fp32 operands: the im2col gather and the exact fp32 GEMM (the project's fp32 rule, DESIGN 2: 2e-4 of the norm)."""
    from sat_amd import ops
    x, dz, prior, ref, bound = _case(SHAPES[2])
    ref32 = (dz.float().double().reshape(-1, dz.shape[3]).T @ _im2col(x.float().double())).reshape(ref.shape)
    dw = ops.conv3x3_wgrad(x.float(), dz.float())
    acc = ops.conv3x3_wgrad(x.float(), dz.float(), out=prior.clone(), accumulate=True)
    torch.cuda.synchronize()
    assert ((dw.double() - ref32).norm() / ref32.norm()).item() <= 2e-4
    assert ((acc.double() - ref32 - prior.double()).norm() / ref32.norm()).item() <= 2e-4
    with pytest.raises(RuntimeError, match="sat_conv3x3_wgrad"):
        ops.conv3x3_wgrad(x.float(), dz.float(), workspace=None)   # the im2col matrix needs the workspace


@pytest.mark.parametrize("cin,cout,dtype", [(64, 128, torch.bfloat16), (128, 192, torch.bfloat16),
                                            (136, 128, torch.bfloat16), (64, 128, torch.float32)])
def test_wgrad_refuses_unsupported_shapes(sat, cin, cout, dtype):
    from sat_amd import ops
    L = sat._lib
    x = torch.zeros(1, 4, 4, cin, dtype=dtype, device=DEV)
    dz = torch.zeros(1, 4, 4, cout, dtype=dtype, device=DEV)
    out = torch.full((cout, 3, 3, cin), 5.0, device=DEV)
    assert ops.conv3x3_wgrad_workspace_bytes(x.shape, cout, dtype) == 0
    code = L.lib().sat_conv3x3_wgrad(1, 4, 4, cin, cout, L.dtype_code(dtype), L.ptr(x), L.ptr(dz), L.ptr(out), 0, None,
                                     0, None, L.stream_of(out))
    assert code == 9001
    with pytest.raises(RuntimeError, match="sat_conv3x3_wgrad"):
        ops.conv3x3_wgrad(x, dz, out=out)
    torch.cuda.synchronize()
    assert (out == 5.0).all()   # nothing ran in its place


def test_wgrad_refuses_a_short_workspace(sat):
    from sat_amd import ops
    x, dz, prior, ref, bound = _case(SHAPES[0])
    pol = sat.Policy(split_k=3)
    need = ops.conv3x3_wgrad_workspace_bytes(x.shape, dz.shape[3], x.dtype, pol)
    assert need > 3 * 9 * 128 * 128 * 4   # three partial tiles per output tile, and the tickets
    short = torch.empty(need - 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="sat_conv3x3_wgrad"):
        ops.conv3x3_wgrad(x, dz, policy=pol, workspace=short)


# =====================================================================================================================
# The trainable tail of the encoder: Encoder.fine_tune(n), its fold kernel, unit backwards, partial plan refresh
# =====================================================================================================================
import ctypes   # noqa: E402

import torch.nn.functional as F   # noqa: E402

from oracle import sat_oracle as O   # noqa: E402

_ENC_PARAMS = {}


def _params(network):
    if network not in _ENC_PARAMS:
        _ENC_PARAMS[network] = O.make_resnet152_params(3) if network == "resnet152" else O.make_vgg19_params(3)
    return _ENC_PARAMS[network]


def _encoder(sat, network, n, dtype):
    enc = sat.Encoder(network, dtype=dtype, fine_tune=n)
    enc.load_state_dict(_params(network))
    return enc.to(DEV)


def _tail_names(network, n):
    if network == "resnet152":
        return [f"net.7.{b}.{m}" for b in (1, 2)[-n:] for m in ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight",
                                                              "bn2.weight", "bn2.bias", "conv3.weight", "bn3.weight",
                                                              "bn3.bias")]
    return [f"net.{i}.{m}" for i in (28, 30, 32, 34)[-n:] for m in ("weight", "bias")]


def _act(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(*shape, generator=g)) * 0.5   # a post-ReLU activation


def _proj(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _ref_tail(network, n, p64, x_nhwc):
    """The oracle's tail in fp64 on an NHWC activation -> features [B, L, D] (autograd-able)."""
    x = x_nhwc.permute(0, 3, 1, 2)
    if network == "resnet152":
        for b in (1, 2)[-n:]:
            pre = f"net.7.{b}"
            out = torch.relu(O._bn(F.conv2d(x, p64[pre + ".conv1.weight"]), p64, pre + ".bn1"))
            out = torch.relu(O._bn(F.conv2d(out, p64[pre + ".conv2.weight"], padding=1), p64, pre + ".bn2"))
            out = O._bn(F.conv2d(out, p64[pre + ".conv3.weight"]), p64, pre + ".bn3")
            x = torch.relu(out + x)
    else:
        for i in (28, 30, 32, 34)[-n:]:
            x = torch.relu(F.conv2d(x, p64[f"net.{i}.weight"], p64[f"net.{i}.bias"], padding=1))
    x = x.permute(0, 2, 3, 1)
    return x.reshape(x.size(0), -1, x.size(-1))


def _ref_grads(network, n, act, R):
    names = _tail_names(network, n)
    p64 = {k: v.double() for k, v in _params(network).items() if v.is_floating_point()}
    for k in names:
        p64[k] = p64[k].clone().requires_grad_(True)
    x = act.double().clone().requires_grad_(True)
    (_ref_tail(network, n, p64, x) * R.double()).sum().backward()
    return {k: p64[k].grad for k in names}, x.grad


def _hip_grads(enc, act, R, dtype):
    x = act.to(DEV).to(dtype).requires_grad_(True)
    k = enc.tail_start()
    feats = enc(x, steps=(k, enc._plan_len()))
    (feats.float() * R.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return {name: p.grad for name, p in enc.named_parameters()}, x.grad, feats


def _assert_fp32_rule(name, got, ref):
    """the error norm within 2e-4 of the gradient's norm, elements within 1e-3 of max |g|."""
    got, ref = got.double().cpu(), ref.double()
    err = (got - ref)
    rel = (err.norm() / ref.norm()).item()
    emax = (err.abs().max() / ref.abs().max()).item()
    print(f"{name}: rel norm {rel:.2e}, max elem {emax:.2e}")
    assert rel <= 2e-4 and emax <= 1e-3, (name, rel, emax)


FP32_CASES = [("resnet152", 2, (2, 7, 7, 2048)), ("vgg19", 4, (2, 14, 14, 512)), ("resnet152", 1, (2, 2, 2, 2048))]


@pytest.mark.parametrize("network,n,shape", FP32_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_unit_backward_fp32_matches_fp64_autograd(sat, network, n, shape):
    enc = _encoder(sat, network, n, torch.float32)
    act = _act(shape, 11)
    R = _proj((shape[0], shape[1] * shape[2], shape[3]), 12)
    grads, dx, feats = _hip_grads(enc, act, R, torch.float32)
    ref, ref_dx = _ref_grads(network, n, act, R)
    names = _tail_names(network, n)
    for name in names:
        _assert_fp32_rule(name, grads[name], ref[name])
    _assert_fp32_rule("input", dx, ref_dx)
    assert all(g is None for k, g in grads.items() if k not in names)


# ---- bf16: an fp64 computation that rounds exactly where the HIP path rounds ----
def _rb(x):
    return x.float().bfloat16().double()


def _hip_activations(enc, act):
    """The tail's forward replayed unit by unit under no_grad: the tensors the backward was handed (the forward is
    deterministic, so these are the saved activations bit for bit; the caller checks the features)."""
    with torch.no_grad():
        x = act.to(DEV)
        plan = enc.compiled_plan(x.device, x.dtype)
        saved = []
        for step in plan[enc.tail_start():]:
            x, sv = enc._tail_unit_forward(x, step)
            saved.append(sv)
    torch.cuda.synchronize()
    return saved


def _mirror(enc, network, saved, dy_bf):
    """Manual fp64 backward over the tail with the HIP path's roundings: the saved activations are the forward's own
    bf16 tensors (``saved``), gradients handed between layers are rounded once to bf16, weight / bias gradients and
    reductions are not rounded.  Reads the folded bf16 weights the encoder itself runs on.  -> ({name: grad}, dx)

    The activations are taken from the forward, not recomputed in fp64: an fp64 forward differs from the fp32-accumulating
    kernels by a few bf16 roundings per layer (measured 2e-4 .. 1.3e-3 of the norm over VGG19's four convs), which flip
    ReLU masks of elements near zero -- each flipped element carries its whole gradient, 2.3e-2 of the norm at
    [2,14,14,512] -- and say nothing about the backward."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    sd = {k: v.double().cpu() for k, v in enc.state_dict().items() if v.is_floating_point()}
    nchw = lambda t: t.double().cpu().permute(0, 3, 1, 2).contiguous()   # noqa: E731
    dy = nchw(dy_bf)
    units = []
    for convs, sv in zip(enc._tail_state, saved):
        fw = [(tc.w_fold.double().cpu().permute(0, 3, 1, 2).contiguous(), tc.b_fold.double().cpu()) for tc in convs]
        units.append((fw,) + tuple(nchw(t) for t in sv))
    grads = {}

    def unfold(prefix_conv, prefix_bn, dwf, dbf):
        w = sd[prefix_conv + ".weight"]
        if prefix_bn is None:
            grads[prefix_conv + ".weight"], grads[prefix_conv + ".bias"] = dwf, dbf
            return
        rstd = 1.0 / torch.sqrt(sd[prefix_bn + ".running_var"] + 1e-5)
        s = sd[prefix_bn + ".weight"] * rstd
        grads[prefix_conv + ".weight"] = dwf * s[:, None, None, None]
        grads[prefix_bn + ".weight"] = rstd * ((dwf * w).sum(dim=(1, 2, 3)) - dbf * sd[prefix_bn + ".running_mean"])
        grads[prefix_bn + ".bias"] = dbf

    n = len(units)
    for i in reversed(range(n)):
        u = units[i]
        if len(u) == 5:
            fw, xin, a1, a2, y = u
            pre = f"net.7.{(1, 2)[-n:][i]}"
            dz3 = dy * (y > 0)
            unfold(pre + ".conv3", pre + ".bn3", conv2d_weight(a2, fw[2][0].shape, dz3), dz3.sum(dim=(0, 2, 3)))
            dz2 = _rb(conv2d_input(a2.shape, fw[2][0], dz3) * (a2 > 0))
            unfold(pre + ".conv2", pre + ".bn2", conv2d_weight(a1, fw[1][0].shape, dz2, padding=1), dz2.sum(dim=(0, 2, 3)))
            dz1 = _rb(conv2d_input(a1.shape, fw[1][0], dz2, padding=1)) * (a1 > 0)
            unfold(pre + ".conv1", pre + ".bn1", conv2d_weight(xin, fw[0][0].shape, dz1), dz1.sum(dim=(0, 2, 3)))
            dy = _rb(conv2d_input(xin.shape, fw[0][0], dz1) + dz3)
        else:
            fw, xin, y = u
            pre = f"net.{(28, 30, 32, 34)[-n:][i]}"
            dz = dy * (y > 0)
            unfold(pre, None, conv2d_weight(xin, fw[0][0].shape, dz, padding=1), dz.sum(dim=(0, 2, 3)))
            dy = _rb(conv2d_input(xin.shape, fw[0][0], dz, padding=1))
    return grads, dy.permute(0, 2, 3, 1)


@pytest.mark.parametrize("network,n,shape", FP32_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_unit_backward_bf16_matches_rounding_mirror(sat, network, n, shape):
    enc = _encoder(sat, network, n, torch.bfloat16)
    act = _act(shape, 21).bfloat16()
    R = _proj((shape[0], shape[1] * shape[2], shape[3]), 22)
    grads, dx, feats = _hip_grads(enc, act.float(), R, torch.bfloat16)
    saved = _hip_activations(enc, act)
    assert torch.equal(saved[-1][-1], feats.detach().view(saved[-1][-1].shape))   # the replay is the forward
    ref, ref_dx = _mirror(enc, network, saved, R.bfloat16().view(shape))
    rels = {}
    for name in _tail_names(network, n) + ["input"]:
        got = (dx if name == "input" else grads[name]).double().cpu()
        want = ref_dx if name == "input" else ref[name]
        rels[name] = ((got - want).norm() / want.norm()).item()
        print(f"{name}: rel norm {rels[name]:.2e}")
    print(f"{network} n={n} {shape}: worst {max(rels.values()):.2e}")
    assert max(rels.values()) <= 1e-2, rels   # the bf16 mirror bound at small shapes


# ---- sat_conv_fold against Encoder._fold ----
@pytest.mark.parametrize("network,n", [("resnet152", 2), ("vgg19", 4)])
def test_conv_fold_matches_the_torch_fold(sat, network, n):
    L = sat._lib
    enc = _encoder(sat, network, n, torch.float32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for unit in enc._tail_units():
        for conv, bn in unit:
            enc.compute_dtype = torch.float32
            w_ref, b_ref, _, _ = enc._fold(conv, bn)
            co, kh, kw, ci = w_ref.shape
            for dtype in (torch.float32, torch.bfloat16):
                wf = torch.empty(co, kh, kw, ci, device=DEV, dtype=dtype)
                bf = torch.empty(co, device=DEV)
                wi = torch.empty(ci, kh, kw, co, device=DEV, dtype=dtype)
                L.check(L.lib().sat_conv_fold(co, ci, kh, kw, L.dtype_code(dtype), L.ptr(conv.weight), L.ptr(conv.bias),
                                              L.ptr(bn.weight if bn else None), L.ptr(bn.bias if bn else None),
                                              L.ptr(bn.running_mean if bn else None),
                                              L.ptr(bn.running_var if bn else None), bn.eps if bn else 0.0, L.ptr(wf),
                                              L.ptr(bf), L.ptr(wi), stream), "sat_conv_fold")
                torch.cuda.synchronize()
                # three roundings of at most one ulp each (sqrt, divide, multiply): relative 2^-22 in fp32
                assert ((bf - b_ref).abs() <= 2.0 ** -22 * b_ref.abs() + 1e-45).all()
                if dtype == torch.float32:
                    assert ((wf - w_ref).abs() <= 2.0 ** -22 * w_ref.abs()).all()
                else:   # within one bf16 ulp of the rounded reference
                    want = w_ref.bfloat16().float()
                    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 1 - 7)
                    assert ((wf.float() - want).abs() <= ulp).all()
                assert torch.equal(wi, wf.flip(1, 2).permute(3, 1, 2, 0).contiguous())


# ---- through the decoder: update, partial refold, equality with a fresh encoder ----
@pytest.mark.parametrize("network,n,shape", [("resnet152", 2, (4, 7, 7, 2048)), ("vgg19", 4, (4, 14, 14, 512))])
def test_train_step_through_the_decoder_and_partial_refold(sat, network, n, shape):
    enc = _encoder(sat, network, n, torch.bfloat16)
    D, V, T = shape[3], 60, 4
    dec = sat.Decoder(V, D, tf=True, ado=network == "resnet152", attention=True)
    dec.load_state_dict(O.make_decoder_params(V, D, 512, network == "resnet152", 5))
    dec = dec.to(DEV).eval()
    caps = O.make_captions(shape[0], T, V, 6).to(DEV)
    act = _act(shape, 31).bfloat16().to(DEV)
    k, end = enc.tail_start(), enc._plan_len()
    tail = enc.tail_parameters()
    tail_ids = {id(p) for p in tail}
    opt = sat.Adam([{"params": list(dec.parameters())}, {"params": tail, "lr": 1e-3}], lr=1e-3)
    with torch.no_grad():
        enc(act, steps=(k, end))
    plan_before = list(enc._plan)
    before = {name: t.clone() for name, t in enc.state_dict().items()}
    feats = enc(act, steps=(k, end))
    preds, alphas = dec(feats, caps)
    loss, _ = sat.caption_loss(preds, alphas, caps)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    names = set(_tail_names(network, n))
    for name, t in enc.state_dict().items():
        if name in names:
            assert not torch.equal(t, before[name]), name        # every tail parameter moved
        else:
            assert torch.equal(t, before[name]), name            # the prefix and every buffer: bit-identical
    with torch.no_grad():
        after = enc(act, steps=(k, end))
    fresh = sat.Encoder(network, dtype=torch.bfloat16, fine_tune=n)
    fresh.load_state_dict(enc.state_dict())
    fresh = fresh.to(DEV)
    with torch.no_grad():
        want = fresh(act, steps=(k, end))
    torch.cuda.synchronize()
    assert torch.equal(after, want)
    assert not torch.equal(after, feats.detach())
    assert all(a is b for a, b in zip(enc._plan[:k], plan_before[:k]))   # the prefix was not rebuilt


# ---- graph capture ----
def test_tail_forward_backward_is_capturable(sat):
    enc = _encoder(sat, "resnet152", 2, torch.bfloat16)
    shape = (2, 7, 7, 2048)
    act = _act(shape, 41).bfloat16().to(DEV)
    R = _proj((2, 49, 2048), 42).bfloat16().to(DEV)
    k, end = enc.tail_start(), enc._plan_len()

    def step():
        feats = enc(act, steps=(k, end))
        feats.backward(R)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in enc.tail_parameters():
        p.grad = None
    step()   # eager: the first backward after grad is None overwrites
    torch.cuda.synchronize()
    eager = enc.tail_grad_flat.clone()
    assert torch.isfinite(eager).all() and eager.abs().sum() > 0
    for p in enc.tail_parameters():
        p.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for _ in range(2):
        enc.tail_grad_flat.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(enc.tail_grad_flat, eager)


# ---- n = 0 is today's encoder ----
def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("network,hw", [("vgg19", 32), ("resnet152", 64)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_fine_tune_zero_is_the_frozen_encoder(sat, network, hw, dtype):
    x = torch.randn(1, 3, hw, hw, generator=torch.Generator().manual_seed(51)).to(DEV)
    a = sat.Encoder(network, dtype=dtype)
    a.load_state_dict(_params(network))
    a = a.to(DEV)
    b = _encoder(sat, network, 0, dtype)
    fa, fb = a(x), b(x)   # grad enabled: nothing is kept, nothing changes
    torch.cuda.synchronize()
    assert torch.equal(fa, fb) and not fb.requires_grad
    assert _same(a._plan, b._plan)
    assert b.tail_start() == len(b._plan) and b.tail_grad_flat is None


# ---- the training CLI ----
def test_train_cli_fine_tunes_the_encoder(sat, tmp_path):
    """train.py --fine-tune-encoder: the prefix runs ahead, the tail trains inside the step, and each epoch saves the
    tuned trunk where model_config.json points generate_caption.py at it."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(repo, "show-attend-and-tell_amd", "train.py"),
                          "--synthetic", "64", "--batch-size", "16", "--epochs", "1", "--max-steps", "2",
                          "--network", "vgg19", "--tf", "--attention", "--vocab", "300", "--log-interval", "1",
                          "--fine-tune-encoder", "2", "--encoder-lr", "1e-3", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert any("train_loss" in r for r in recs) and any("val_bleu4" in r for r in recs)
    tuned_path = tmp_path / "encoder_vgg19_1.pth"
    assert tuned_path.exists() and (tmp_path / "model_vgg19_1.pth").exists()
    cfg = json.load(open(tmp_path / "model_config.json"))
    assert cfg["encoder_weights"] == os.path.abspath(tuned_path) and cfg["fine_tune_encoder"] == 2
    start = torch.load(tmp_path / "encoder_vgg19.pth", weights_only=True)
    tuned = torch.load(tuned_path, weights_only=True)
    assert list(start) == list(tuned)
    moved = {k for k in start if not torch.equal(start[k], tuned[k])}
    assert moved == {"net.32.weight", "net.32.bias", "net.34.weight", "net.34.bias"}, sorted(moved)
    assert all(torch.isfinite(v).all() for v in tuned.values())

"""dL/d(img_features) of sat_amd.Decoder on the GPU (sat_decoder_backward_features) against the CPU oracle's
``feats.grad`` (oracle.sat_oracle.decoder_forward + caption_loss, the reference's loss.backward() through
decoder.py / attention.py into the encoder output, encoder.py:13-17).

Cases are built by tests/test_gpu_shapes.py's ``_make_case`` (post-ReLU features rounded to bf16).  fp32 follows
the parameter-gradient rule of ``_assert_fp32``: the norm within max(2e-4, 2 x noise) of the reference norm and
every element within max(1e-3 max|g|, 2 x elementwise noise), the noise being the oracle's own fp32 / fp64 gap.
bf16 is measured against the bf16 rounding mirror in fp64 (relative error norm, bound 1e-2: the project's B = 4
mirror bound; the gradient is returned in bf16, whose rounding alone is 1.6-1.7e-3 of the norm).
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import sat_oracle as O
from test_gpu_shapes import _make_case

pytestmark = pytest.mark.gpu
DEV = "cuda"

# name: (B, L, D, V, T, tf, ado, attention, bert)
CASES = {
    "att_ado_tf": (3, 16, 64, 60, 9, True, True, True, False),
    "att_simple_greedy": (2, 12, 48, 50, 8, False, False, True, False),
    "noatt_ado_tf": (3, 16, 64, 60, 9, True, True, False, False),
    "noatt_simple_greedy": (2, 12, 48, 50, 8, False, False, False, False),
    "bert_att_simple_tf": (2, 16, 32, 128, 10, True, False, True, True),
    "resnet_like": (4, 49, 2048, 60, 4, True, True, True, False),
    "vgg_like": (4, 196, 512, 60, 4, True, False, True, False),
    "long_caption": (2, 12, 48, 50, 131, True, False, True, False),
    "shortest_caption": (2, 16, 64, 60, 3, True, True, True, False),
}
MIRROR_CASES = list(CASES)[:7]
MIRROR_TOL = 1e-2


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


@functools.lru_cache(maxsize=None)
def _case(name):
    B, L, D, V, T, tf, ado, att, bert = CASES[name]
    c = _make_case(D, L, 768 if bert else 512, V, T, tf, ado, bert, B, 31 + list(CASES).index(name))
    c["att"] = att
    c["name"] = name
    return c


def _decoder(sat, c):
    kw = dict(tf=c["tf"], ado=c["ado"], bert=c["bert"], attention=c["att"])
    if c["bert"]:
        dec = sat.Decoder(c["V"], c["D"], bert_embedding_weight=c["p"]["embedding.weight"], **kw)
    else:
        dec = sat.Decoder(c["V"], c["D"], **kw)
    dec.load_state_dict(c["p"], strict=True)
    return dec.to(DEV)


def _hip(sat, c, dtype, policy=None, train=True, requires=True, hook=False, dec=None):
    """One seeded step on the HIP path; the feature gradient and everything a caller compares."""
    dec = dec if dec is not None else _decoder(sat, c)
    dec.train(train)
    dec.policy = policy
    if train:
        dec.dropout_mask = c["masks"].permute(1, 0, 2).contiguous().to(torch.uint8)
    if hook:
        dec._grad_hooks.append(lambda phase, d: None)
    for p in dec.parameters():
        p.grad = None
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).to(dtype).requires_grad_(requires)
    preds, alphas = dec(feats, caps)
    pad, skip = sat.special_ids(c["bert"])
    loss, _ = sat.caption_loss(preds, alphas, caps, 1.0, pad, skip)
    loss.backward()
    torch.cuda.synchronize()
    out = dict(preds=preds.detach().clone(), alphas=alphas.detach().clone(), flat=dec._grad_flat.clone(),
               tokens=dec.last_tokens.long().cpu(), grad=None if feats.grad is None else feats.grad.detach().clone(),
               dec=dec, feats=feats, caps=caps)
    if requires:
        assert feats.grad is not None and feats.grad.dtype == dtype and feats.grad.shape == feats.shape
    return out


def _oracle_grad(c, dtype, fed=None, train=True, mirror=False):
    """feats.grad of the oracle; ``fed``: teacher-forced on the tokens the HIP decoder fed itself (greedy feedback is a
    constant for autograd: ``_oracle_fed`` of tests/test_gpu_shapes.py), the loss still scoring the real captions."""
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    feats = c["feats"].to(dtype).clone().requires_grad_(True)
    caps_in = c["caps"]
    if fed is not None:
        caps_in = c["caps"].clone()
        caps_in[:, :c["T"] - 1] = fed.to(caps_in.dtype)
    with (O.bf16_mirror() if mirror else contextlib.nullcontext()):
        preds, alphas, _ = O.decoder_forward(p, feats, caps_in, tf=True if fed is not None else c["tf"], ado=c["ado"],
                                             attention=c["att"], bert=c["bert"], training=train,
                                             dropout_masks=c["masks"].to(dtype) if train else None)
        O.caption_loss(preds, alphas, c["caps"]).backward()
    return feats.grad.detach()


@functools.lru_cache(maxsize=None)
def _oracle_tf(name, dtype, train=True, mirror=False):
    """Shared, unchanged references of the teacher-forced cases."""
    return _oracle_grad(_case(name), dtype, None, train, mirror)


def _refs(c, h, dtype, train=True, mirror=False):
    if c["tf"]:
        return _oracle_tf(c["name"], dtype, train, mirror)
    return _oracle_grad(c, dtype, h["tokens"], train, mirror)


def _assert_rule(g, ref, r64, label):
    """The fp32 gradient rule of tests/test_gpu_shapes.py's _assert_fp32."""
    g, ref, r64 = (x.reshape(-1).double().cpu() for x in (g, ref, r64))
    ref_norm = ref.norm().item()
    assert ref_norm > 1e-7, label
    noise_norm = abs(r64.norm().item() - ref_norm) / ref_norm
    noise_elem = (r64 - ref).abs().max().item()
    d_norm = abs(g.norm().item() - ref_norm) / ref_norm
    err = (g - ref).abs().max().item()
    gmax = g.abs().max().item()
    print(f"{label}: norm diff {d_norm:.3e} (noise {noise_norm:.3e}), elem err / max|g| {err / gmax:.3e} "
          f"(noise {noise_elem / gmax:.3e})")
    assert d_norm <= max(2e-4, 2 * noise_norm), label
    assert err <= max(1e-3 * gmax, 2 * noise_elem) + 1e-9, label


def _instance(sat, h):
    L = sat._lib
    out = (ctypes.c_int * 8)()
    dec = h["dec"]
    L.check(L.lib().sat_decoder_instance(ctypes.byref(dec._dims(h["feats"], h["caps"])), ctypes.byref(dec._layout()),
                                         out, 8), "sat_decoder_instance")
    return list(out)


# ---------------------------------------------------------------- 1. the kernel alone
KERNEL_SHAPES = [(1, 1, 8, 2), (3, 16, 64, 8), (2, 49, 2048, 3), (2, 196, 512, 7), (2, 12, 48, 130), (2, 1024, 8, 2)]


@pytest.mark.parametrize("with_mean", [True, False], ids=["mean", "nomean"])
@pytest.mark.parametrize("with_addend", [True, False], ids=["addend", "noaddend"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accumulate_kernel_matches_einsum(sat, shape, with_addend, with_mean):
    B, L, D, T1 = shape
    L_ = sat._lib
    g = torch.Generator().manual_seed(B * 1000 + L + D + T1)
    alpha = torch.softmax(torch.randn(B, T1, L, generator=g), 2)
    # dctx rows at twice their width for one shape: the kernel takes the strides it is given
    pad = 2 if shape == (3, 16, 64, 8) else 1
    dctx_full = torch.randn(B, T1, pad * D, generator=g)
    dctx = dctx_full[..., :D]
    addend = torch.randn(B * L, D, generator=g) if with_addend else None
    mean = torch.randn(B, D, generator=g) if with_mean else None
    ref = torch.einsum("btl,btd->bld", alpha.double(), dctx.double())
    if with_mean:
        ref = ref + (mean.double() / L).unsqueeze(1)
    if with_addend:
        ref = ref + addend.double().view(B, L, D)
    scale = ref.abs().max().item()
    dev = [None if x is None else x.to(DEV) for x in (alpha, dctx_full, addend, mean)]
    for dtype in (torch.float32, torch.bfloat16):
        out = torch.full((B, L, D), float("nan"), device=DEV, dtype=dtype)
        L_.check(L_.lib().sat_feature_grad_accumulate(
            B, L, D, T1, L_.dtype_code(dtype), L_.ptr(dev[0]), T1 * L, L, L_.ptr(dev[1]), T1 * pad * D, pad * D,
            L_.ptr(dev[2]), D, L_.ptr(dev[3]), D, L_.ptr(out), D, L_.stream_of(out)), "sat_feature_grad_accumulate")
        torch.cuda.synchronize()
        got = out.double().cpu()
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        if dtype == torch.float32:
            assert err.max().item() <= 1e-5 * scale, err.max().item() / scale
        else:   # one bf16 rounding of the fp32 sum
            assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-5 * scale).all()), (err / scale).max().item()


# ---------------------------------------------------------------- 2. fp32 parity
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_matches_oracle(sat, name):
    c = _case(name)
    h = _hip(sat, c, torch.float32)
    _assert_rule(h["grad"], _refs(c, h, torch.float32), _refs(c, h, torch.float64), name)


FORMS = {"split": dict(), "one_chunk": dict(attn_bwd_chunks=1), "two_launch": dict(attn_bwd=1)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["resnet_like", "vgg_like"])
def test_fp32_attention_backward_forms(sat, name, form):
    """The dL/dcontext store in each attention backward: split over several chunks per row (chunk 0 stores), one
    workgroup per row, and the two-launch form."""
    c = _case(name)
    h = _hip(sat, c, torch.float32, policy=sat.Policy(**FORMS[form]) if FORMS[form] else None)
    chunks = _instance(sat, h)[4]
    assert {"split": chunks > 1, "one_chunk": chunks == 1, "two_launch": chunks == 0}[form], chunks
    _assert_rule(h["grad"], _refs(c, h, torch.float32), _refs(c, h, torch.float64), f"{name}/{form}")


def test_fp32_eval_mode(sat):
    c = _case("att_ado_tf")
    h = _hip(sat, c, torch.float32, train=False)
    _assert_rule(h["grad"], _refs(c, h, torch.float32, train=False), _refs(c, h, torch.float64, train=False),
                 "att_ado_tf/eval")


# ---------------------------------------------------------------- 3. bf16 against the rounding mirror
@pytest.mark.parametrize("name", MIRROR_CASES)
def test_bf16_close_to_rounding_mirror(sat, name):
    """Measured on an MI355X (relative error norm of the bf16 feats.grad against the fp64 mirror): see DESIGN.md
    section 4.12 for the figures per case."""
    c = _case(name)
    h = _hip(sat, c, torch.bfloat16)
    ref = _refs(c, h, torch.float64, mirror=True)
    g = h["grad"].double().cpu()
    err = ((g - ref).norm() / ref.norm()).item()
    print(f"{name}: bf16 feats.grad vs mirror, relative error norm {err:.3e}")
    assert err <= MIRROR_TOL, err


# ---------------------------------------------------------------- 4. not requested means unchanged
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["att_ado_tf", "noatt_ado_tf", "resnet_like"])
def test_not_requested_means_unchanged(sat, name, dtype):
    c = _case(name)
    on = _hip(sat, c, dtype, requires=True)
    off = _hip(sat, c, dtype, requires=False)
    assert off["grad"] is None and on["grad"] is not None
    assert torch.equal(on["preds"], off["preds"])
    assert torch.equal(on["alphas"], off["alphas"])
    dec = on["dec"]
    params = dict(dec.named_parameters())
    for n in dec.active_param_names():
        o, m = dec._offsets[n], params[n].numel()
        assert torch.equal(on["flat"][o:o + m], off["flat"][o:o + m]), n


# ---------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("name", ["att_ado_tf", "resnet_like", "noatt_ado_tf"])
def test_bf16_deterministic(sat, name):
    c = _case(name)
    a, b = _hip(sat, c, torch.bfloat16), _hip(sat, c, torch.bfloat16)
    assert torch.equal(a["grad"], b["grad"])


# ---------------------------------------------------------------- 6. graph capture
def test_captured_backward_rewrites_feature_grad(sat):
    c = _case("att_ado_tf")
    dec = _decoder(sat, c).eval()
    caps = c["caps"].to(DEV)
    eager_feats = c["feats"].to(DEV).bfloat16().requires_grad_(True)
    preds, alphas = dec(eager_feats, caps)
    loss, _ = sat.caption_loss(preds, alphas, caps)
    loss.backward()
    torch.cuda.synchronize()
    eager = eager_feats.grad.clone()
    for p in dec.parameters():
        p.grad = None
    feats = c["feats"].to(DEV).bfloat16().requires_grad_(True)   # static input, .grad None before the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preds, alphas = dec(feats, caps)
        loss, _ = sat.caption_loss(preds, alphas, caps)
        loss.backward()
    assert feats.grad is not None
    for _ in range(2):
        feats.grad.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(feats.grad, eager)


# ---------------------------------------------------------------- 7. chain rule
def test_chain_rule_into_a_projection(sat):
    """feats = relu(x A) in torch on the device with A requiring grad: what an adapter between a frozen trunk and
    the decoder trains on."""
    c = _case("att_ado_tf")
    B, L, D = c["feats"].shape
    K = 24
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, L, K, generator=g)
    A0 = torch.randn(K, D, generator=g) / K ** 0.5

    def oracle(dtype):
        p = {k: v.to(dtype) for k, v in c["p"].items()}
        A = A0.to(dtype).clone().requires_grad_(True)
        feats = torch.relu(x.to(dtype) @ A)
        preds, alphas, _ = O.decoder_forward(p, feats, c["caps"], tf=True, ado=True, attention=True, training=True,
                                             dropout_masks=c["masks"].to(dtype))
        O.caption_loss(preds, alphas, c["caps"]).backward()
        return A.grad.detach()

    dec = _decoder(sat, c).train()
    dec.dropout_mask = c["masks"].permute(1, 0, 2).contiguous().to(torch.uint8)
    A = A0.to(DEV).requires_grad_(True)
    feats = torch.relu(x.to(DEV) @ A)
    caps = c["caps"].to(DEV)
    preds, alphas = dec(feats, caps)
    loss, _ = sat.caption_loss(preds, alphas, caps)
    loss.backward()
    torch.cuda.synchronize()
    assert A.grad is not None
    _assert_rule(A.grad, oracle(torch.float32), oracle(torch.float64), "A.grad")


# ---------------------------------------------------------------- 8. phases
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["att_ado_tf", "noatt_ado_tf"])
def test_two_phase_backward_is_bit_identical(sat, name, dtype):
    c = _case(name)
    one = _hip(sat, c, dtype)
    two = _hip(sat, c, dtype, hook=True)
    assert torch.equal(one["grad"], two["grad"])
    assert torch.equal(one["flat"], two["flat"])


def test_deferred_backward_refuses_features_that_require_grad(sat):
    c = _case("att_ado_tf")
    dec = _decoder(sat, c).eval()
    dec.defer_recurrent_backward(True)
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match="defer_recurrent_backward"):
        dec(feats, caps)
    # features that do not require grad still run deferred
    preds, alphas = dec(feats.detach(), caps)
    loss, _ = sat.caption_loss(preds, alphas, caps)
    loss.backward()
    dec.finish_backward()
    torch.cuda.synchronize()
    assert dec.init_h.weight.grad is not None

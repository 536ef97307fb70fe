"""Scheduled sampling (sat_decoder_forward_sampled, Decoder.tf_prob): at every step t >= 1 a row feeds its caption's
token where its keep bit is set and the previous step's argmax elsewhere (decoder.py:108-112 / 131-133 mixed per token).

Forms: the fused greedy loop (bf16; the select inside the LSTM kernel's token fold) and the per-op loop (fp32, and bf16
under Policy(greedy_step=1); the select form of the argmax kernel).  The fed tokens are constants for autograd, so the
references are those of the greedy tests: the oracle teacher-forced on the tokens the HIP decoder fed
(test_gpu_shapes._oracle_fed) under test_gpu_shapes' fp32 rule, the bf16 rounding mirror under test_gpu_greedy's
bounds, test_gpu_feature_grad's rule for the feature gradient -- all imported, none restated.

Shapes: B = 3 / 4, T = 6-8, the smallest at which each path differs -- E = 128 (two workgroups of the LSTM kernel per
row must agree on the token; the module fixes E = 512, so a test-local subclass rebuilds the submodules), E = 512 (the
LDS-staged head), V = 1003 (odd: the head's scalar stores), V = 2600, L = 196, BERT (E = 768, V = 30522, start token
101), the simple and the ado head, one case without attention.
"""
import ctypes
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import sat_oracle as O
import sched_sampling_host as H
import test_gpu_feature_grad as FG
import test_gpu_greedy as G
import test_gpu_shapes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "show-attend-and-tell_amd")

CASES = {
    # name: (D, L, E, V, T, ado, bert, attention, B)
    "e128_ado": (512, 49, 128, 1003, 6, True, False, True, 3),
    "e512_ado_v1003": (512, 49, 512, 1003, 6, True, False, True, 3),
    "e512_simple_l196": (512, 196, 512, 2600, 8, False, False, True, 4),
    "bert": (512, 49, 768, 30522, 6, False, True, True, 3),
    "no_attention": (512, 49, 512, 1003, 7, True, False, False, 4),
}
ORACLE_CASES = [n for n in CASES if n != "no_attention"]   # _oracle_fed runs the attention decoder
FORMS = {"fused": (torch.bfloat16, 0), "perop_bf16": (torch.bfloat16, 1), "perop_fp32": (torch.float32, 0)}


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


_CASE = {}


def _case(name):
    if name not in _CASE:
        D, Lf, E, V, T, ado, bert, att, Bn = CASES[name]
        c = S._make_case(D, Lf, E, V, T, False, ado, bert, Bn, 61 + list(CASES).index(name))
        c["att"], c["name"], c["B"] = att, name, Bn
        # the injected keep mask: Bernoulli(0.5) from a fixed generator (column 0 is ignored by the kernels)
        c["keep"] = torch.from_numpy((np.random.default_rng(7 + Bn + T).random((Bn, T - 1)) < 0.5).astype(np.uint8))
        _CASE[name] = c
    return _CASE[name]


def _decoder(sat, c):
    """The module of a case; E other than the module's own (512, BERT 768): the submodules rebuilt at that size before
    the first forward lays out the flat buffer."""
    if c["bert"] or c["E"] == 512:
        return FG._decoder(sat, c)
    E, D, V = c["E"], c["D"], c["V"]
    dec = sat.Decoder(V, D, tf=False, ado=c["ado"], bert=False, attention=c["att"])
    dec.embedding_size = E
    dec.embedding = nn.Embedding(V, E)
    dec.init_h, dec.init_c, dec.f_beta = nn.Linear(D, E), nn.Linear(D, E), nn.Linear(E, D)
    dec.attention = sat.Attention(D, E)
    dec.lstm = nn.LSTMCell(E + D, E)
    if c["ado"]:
        dec.f_h, dec.f_z, dec.f_out = nn.Linear(E, E), nn.Linear(D, E), nn.Linear(E, V)
    dec.deep_output = nn.Linear(E, V)
    dec.load_state_dict(c["p"], strict=True)
    return dec.to(DEV)


_RUNS = {}


def _run(sat, name, form, mode, feats_grad=False, adam=False):
    """One seeded train-mode step (injected dropout mask) of a case in one form.  mode: 'mask' (the case's injected keep
    mask), 'zeros' / 'ones' (injected), 'p0' / 'p1' (the draw), 'greedy' (tf_prob None, tf False), 'tf' (tf_prob None,
    tf True).  Cached: the results are shared and left unchanged."""
    key = (name, form, mode, feats_grad, adam)
    if key in _RUNS:
        return _RUNS[key]
    c = _case(name)
    dtype, step = FORMS[form]
    dec = _decoder(sat, c).train()
    dec.policy = sat.Policy(greedy_step=step) if step else None
    dec.dropout_mask = c["masks"].permute(1, 0, 2).contiguous().to(torch.uint8)
    B, T1 = c["B"], c["T"] - 1
    if mode == "mask":
        dec.tf_prob, dec.tf_mask = 0.5, c["keep"].clone()
    elif mode in ("zeros", "ones"):
        dec.tf_prob, dec.tf_mask = 0.5, torch.full((B, T1), int(mode == "ones"), dtype=torch.uint8)
    elif mode in ("p0", "p1"):
        dec.tf_prob = float(mode == "p1")
    elif mode == "tf":
        dec.use_tf = True
    opt = sat.Adam(dec.parameters(), lr=S.LR)
    opt.zero_grad()
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).to(dtype).requires_grad_(feats_grad)
    preds, alphas = dec(feats, caps)
    pad, skip = sat.special_ids(c["bert"])
    loss, _ = sat.caption_loss(preds, alphas, caps, 1.0, pad, skip)
    loss.backward()
    torch.cuda.synchronize()
    params = dict(dec.named_parameters())
    h = dict(loss=loss.item(), preds=preds.detach().float().cpu(), alphas=alphas.detach().float().cpu(),
             grads={n: params[n].grad.detach().float().cpu().clone() for n in dec.active_param_names()},
             tokens=dec.last_tokens.long().cpu(),
             keep=None if dec.last_tf_mask is None else dec.last_tf_mask.cpu(),
             feat_grad=None if feats.grad is None else feats.grad.detach().float().cpu())
    if adam:
        opt.step()
        torch.cuda.synchronize()
        h["params"] = {n: params[n].detach().float().cpu().clone() for n in h["grads"]}
    _RUNS[key] = h
    return h


def _start(c):
    return 101 if c["bert"] else 0


def _assert_fed_tokens(c, h, keep_expected=None):
    """tokens = captions where keep, the argmax of the stored logits of step t - 1 elsewhere; bit-exact"""
    T1 = c["T"] - 1
    tok, keep = h["tokens"], h["keep"].bool()
    assert torch.equal(tok[:, 0], torch.full_like(tok[:, 0], _start(c)))
    assert bool(h["keep"][:, 0].eq(1).all())
    if keep_expected is not None:
        want = keep_expected.clone()
        want[:, 0] = 1
        assert torch.equal(h["keep"], want)
    am = h["preds"].argmax(2)   # first index on ties (decoder.py:132)
    want_tok = torch.where(keep[:, 1:], c["caps"][:, 1:T1], am[:, :T1 - 1])
    assert torch.equal(tok[:, 1:], want_tok)


# ------------------------------------------------------------------ 1. self-consistency of the fed tokens
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_fed_tokens_follow_the_mask(sat, name, form):
    c = _case(name)
    h = _run(sat, name, form, "mask")
    _assert_fed_tokens(c, h, c["keep"])
    k = h["keep"][:, 1:]
    assert 0 < int(k.sum()) < k.numel()   # the case exercises both sources


# ------------------------------------------------------------------ 2. values and gradients
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_fp32_matches_the_fed_token_oracle(sat, name):
    c = _case(name)
    h = _run(sat, name, "perop_fp32", "mask", adam=True)
    o32, o64 = S._oracle_fed(c, h["tokens"], torch.float32), S._oracle_fed(c, h["tokens"], torch.float64)
    # test_gpu_shapes' fp32 rule against a reference that feeds given tokens (its teacher-forced branch: the fed-token
    # oracle is one): preds / alphas / loss 1e-4, gradients by the fp64 noise gauge, fused Adam
    S._assert_fp32(dict(c, tf=True), h, o32, o64)


@pytest.mark.parametrize("form", ["fused", "perop_bf16"])
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_bf16_matches_the_fed_token_mirror(sat, name, form):
    c = _case(name)
    h = _run(sat, name, form, "mask")
    G._assert_mirror(h, G._mirror_fed(c, h["tokens"]))


def test_feature_gradient_fp32(sat):
    name = "e512_ado_v1003"
    c = _case(name)
    h = _run(sat, name, "perop_fp32", "mask", feats_grad=True)
    _assert_fed_tokens(c, h, c["keep"])
    ref = FG._oracle_grad(c, torch.float32, fed=h["tokens"])
    r64 = FG._oracle_grad(c, torch.float64, fed=h["tokens"])
    FG._assert_rule(h["feat_grad"], ref, r64, "sampled feature gradient")


def test_feature_gradient_bf16_fused(sat):
    name = "e512_ado_v1003"
    c = _case(name)
    h = _run(sat, name, "fused", "mask", feats_grad=True)
    ref = FG._oracle_grad(c, torch.float64, fed=h["tokens"], mirror=True).float()
    err = ((h["feat_grad"] - ref).norm() / ref.norm()).item()
    print(f"bf16 sampled feature gradient vs the mirror: {err:.3e}")
    assert err <= FG.MIRROR_TOL, err


# ------------------------------------------------------------------ 3. the ends
@pytest.mark.parametrize("source", ["zeros", "p0"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_keep_nothing_is_the_greedy_step_bit_for_bit(sat, name, form, source):
    h, g = _run(sat, name, form, source), _run(sat, name, form, "greedy")
    assert bool(h["keep"][:, 1:].eq(0).all()) and bool(h["keep"][:, 0].eq(1).all())
    assert g["keep"] is None
    assert torch.equal(h["tokens"], g["tokens"])
    assert torch.equal(h["preds"], g["preds"]) and torch.equal(h["alphas"], g["alphas"])
    assert h["loss"] == g["loss"]
    assert sorted(h["grads"]) == sorted(g["grads"])
    for n in g["grads"]:
        assert torch.equal(h["grads"][n], g["grads"][n]), n


@pytest.mark.parametrize("source", ["ones", "p1"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_keep_everything_is_teacher_forcing(sat, name, form, source):
    c = _case(name)
    T1 = c["T"] - 1
    h = _run(sat, name, form, source)
    assert bool(h["keep"].eq(1).all())
    want = c["caps"][:, :T1].clone()
    assert torch.equal(h["tokens"], want)
    if FORMS[form][0] == torch.float32:   # the README's parity rule against the same decoder's tf = True forward
        t = _run(sat, name, form, "tf")
        assert torch.equal(t["tokens"], want)
        assert S.rel(h["preds"], t["preds"]) < 1e-4
        assert S.rel(h["alphas"], t["alphas"]) < 1e-4
    elif c["att"]:   # the mirror teacher-forced on the captions, the bounds of test_bf16_matches_the_fed_token_mirror
        G._assert_mirror(h, G._mirror_fed(c, h["tokens"]))


# ------------------------------------------------------------------ 4. the draw
DRAW = dict(B=64, T=21, E=128, V=200, D=64, L=16, p=0.25)


def _draw_decoder(sat, form):
    torch.manual_seed(4321)   # the module's seed comes from torch's generator
    c = dict(E=DRAW["E"], D=DRAW["D"], V=DRAW["V"], ado=True, att=True, bert=False,
             p=O.make_decoder_params(DRAW["V"], DRAW["D"], DRAW["E"], True, 5))
    dec = _decoder(sat, c).train()
    dec.policy = sat.Policy(greedy_step=1) if form == "perop_bf16" else None
    dec.tf_prob = DRAW["p"]
    return dec


def _draw_forward(dec, feats, caps):
    with torch.no_grad():
        dec(feats, caps)
    torch.cuda.synchronize()
    return dec.last_tf_mask.cpu().numpy().copy(), dec.last_tokens.long().cpu()


def test_seeded_draw_matches_the_host_restatement(sat):
    B, T, p = DRAW["B"], DRAW["T"], DRAW["p"]
    rng = np.random.default_rng(3)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, DRAW["L"], DRAW["D"])), 0).astype(np.float32))
    caps = O.make_captions(B, T, DRAW["V"], 9).to(DEV)
    first, second = {}, {}
    for form in ("fused", "perop_bf16", "perop_fp32"):
        dec = _draw_decoder(sat, form)
        f = feats.to(DEV).to(FORMS[form][0])
        first[form], tok = _draw_forward(dec, f, caps)
        host = H.host_tf_mask(H.step_seed(dec._seed_host, 0), B, T - 1, p)
        assert np.array_equal(first[form], host), form
        keep = torch.from_numpy(first[form]).bool()
        assert torch.equal(tok[:, 1:][keep[:, 1:]], caps.cpu()[:, 1:T - 1][keep[:, 1:]])
        second[form], _ = _draw_forward(dec, f, caps)   # the counter advanced: another draw, the host's for counter 1
        assert not np.array_equal(second[form], first[form])
        assert np.array_equal(second[form], H.host_tf_mask(H.step_seed(dec._seed_host, 1), B, T - 1, p))
    assert np.array_equal(first["fused"], first["perop_bf16"]) and np.array_equal(first["fused"], first["perop_fp32"])
    assert np.array_equal(second["fused"], second["perop_bf16"])
    m = first["fused"][:, 1:]
    n = m.size
    assert n == 64 * 19
    assert abs(m.mean() - p) <= 5 * math.sqrt(p * (1 - p) / n), m.mean()   # the binomial bound, 0.062
    assert (m.std(axis=0) > 0).all() and (m.std(axis=1) > 0).any()
    # two modules built under the same torch.manual_seed draw the same first mask
    f = feats.to(DEV).bfloat16()
    a = _draw_decoder(sat, "fused")
    ma, _ = _draw_forward(a, f, caps)
    b = _draw_decoder(sat, "fused")
    mb, _ = _draw_forward(b, f, caps)
    assert a._seed_host == b._seed_host and np.array_equal(ma, mb) and np.array_equal(ma, first["fused"])


# ------------------------------------------------------------------ 5. graph capture and the device scalar
def test_captured_step_follows_the_device_scalar(sat):
    name = "e512_simple_l196"
    c = _case(name)
    T1 = c["T"] - 1
    torch.manual_seed(77)
    dec = _decoder(sat, c).train()
    dec.dropout_mask = c["masks"].permute(1, 0, 2).contiguous().to(torch.uint8).to(DEV)
    scalar = torch.tensor([0.5], device=DEV, dtype=torch.float32)
    dec.tf_prob, dec.tf_prob_tensor = 0.5, scalar
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).bfloat16()
    pad, skip = sat.special_ids(c["bert"])
    dec(feats, caps)   # eager warm-up: draws the host seed, builds the flat buffers
    torch.cuda.synchronize()
    for p in dec.parameters():
        p.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preds, alphas = dec(feats, caps)
        loss, _ = sat.caption_loss(preds, alphas, caps, 1.0, pad, skip)
        loss.backward()
    tokens, keep = dec.last_tokens, dec.last_tf_mask

    def replay(p, counter=None):
        scalar.fill_(p)
        if counter is not None:
            dec._seed_dev.fill_(counter)
        g.replay()
        torch.cuda.synchronize()
        return tokens.long().cpu(), keep.cpu().clone(), preds.detach().float().cpu(), dec._grad_flat.clone()

    tok, k, _, _ = replay(1.0)
    assert torch.equal(tok, c["caps"][:, :T1]) and bool(k.eq(1).all())
    tok, k, pr, _ = replay(0.0)
    e = _run(sat, name, "fused", "p0")   # the eager p = 0 forward (a host float, no device scalar)
    assert bool(k[:, 1:].eq(0).all())
    assert torch.equal(tok, e["tokens"]) and torch.equal(pr, e["preds"])
    assert torch.equal(tok[:, 1:], pr.argmax(2)[:, :-1])
    _, k1, _, _ = replay(0.5)
    _, k2, _, _ = replay(0.5)
    assert not torch.equal(k1, k2)   # 28 fresh Bernoulli(0.5) draws per replay
    _, ka, _, ga = replay(0.5, counter=5)
    _, kb, _, gb = replay(0.5, counter=5)
    assert torch.equal(ka, kb) and torch.equal(ga, gb)
    assert np.array_equal(ka.numpy(), H.host_tf_mask(H.step_seed(dec._seed_host, 5), c["B"], T1, 0.5))


# ------------------------------------------------------------------ 6. refusals
def test_refusals_and_eval_mode(sat):
    name = "e512_ado_v1003"
    c = _case(name)
    dec = _decoder(sat, c).train()
    for bad in (-0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            dec.tf_prob = bad
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).bfloat16()
    dec.tf_prob = 0.5
    dec.tf_mask = torch.ones(c["B"], c["T"], dtype=torch.uint8)   # [B, T]: one column too many
    with pytest.raises(ValueError, match="tf_mask"):
        dec(feats, caps)
    dec.tf_mask = None
    # the C entry refuses teacher-forcing dims and a probability outside [0, 1]
    L = sat._lib
    dims = dec._dims(feats, caps)
    lay = dec._layout()
    ws_bytes = L.lib().sat_decoder_workspace_bytes(ctypes.byref(dims))
    ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
    preds = torch.empty(c["B"], c["T"] - 1, c["V"], device=DEV, dtype=torch.bfloat16)
    alphas = torch.empty(c["B"], c["T"] - 1, c["L"], device=DEV, dtype=torch.float32)
    mask = torch.ones(c["B"], c["T"] - 1, c["E"], device=DEV, dtype=torch.uint8)
    dims.has_dropout_mask = 1

    def call(p):
        return L.lib().sat_decoder_forward_sampled(ctypes.byref(dims), ctypes.byref(lay), L.ptr(dec._flat),
                                                   L.ptr(dec._flat_lp), L.ptr(feats), L.ptr(caps), L.ptr(mask), p, None,
                                                   None, None, L.ptr(ws), ws_bytes, L.ptr(preds), L.ptr(alphas), None,
                                                   L.stream_of(preds))
    dims.tf = 1
    assert call(0.5) == 9001
    dims.tf = 0
    assert call(1.5) == 9001 and call(-0.1) == 9001
    assert call(0.5) == 0
    torch.cuda.synchronize()
    # eval mode ignores tf_prob: the reference's tf flag governs, bit for bit
    dec.eval()
    with torch.no_grad():
        dec.tf_prob = 0.3
        p1, a1 = dec(feats, caps)
        t1, k1 = dec.last_tokens.clone(), dec.last_tf_mask
        dec.tf_prob = None
        p0, a0 = dec(feats, caps)
    torch.cuda.synchronize()
    assert k1 is None
    assert torch.equal(p1, p0) and torch.equal(a1, a0) and torch.equal(t1, dec.last_tokens)


# ------------------------------------------------------------------ 7. end to end
def test_train_cli_with_a_decaying_schedule(sat, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--synthetic", "64", "--tf-prob", "0.75",
                        "--tf-prob-end", "0.25", "--epochs", "2", "--max-steps", "3", "--batch-size", "16",
                        "--network", "vgg19", "--ado", "--attention", "--vocab", "200", "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [x["tf_prob"] for x in recs if "tf_prob" in x] == [0.75, 0.25]
    assert all(math.isfinite(x["train_loss"]) for x in recs if "train_loss" in x)
    cfg = json.load(open(tmp_path / "model_config.json"))
    assert cfg["tf_prob"] == 0.75 and cfg["tf_prob_end"] == 0.25 and cfg["tf"] is False
    spec = importlib.util.spec_from_file_location("sat_caption_cli_ss", os.path.join(PKG, "generate_caption.py"))
    gc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gc)
    _, decoder, _, _ = gc.load_model(str(tmp_path / "model_vgg19_2.pth"))
    assert decoder.tf_prob is None and not decoder.training

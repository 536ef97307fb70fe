"""Sampled feedback and the token-weighted loss (sat_decoder_forward_sample, sat_sample_noise,
sat_caption_loss_weighted_*; Decoder.sample, sat_amd.weighted_caption_loss): the hot path of self-critical sequence
training.

The draw is a stated function, sampled[b, t] = argmax_v(preds[b, t, v] + tau * G(seed, b, t, v)), so the tests restate it
from the stored logits and the noise sat_sample_noise reports, bit for bit, in both loop forms (the fused greedy loop:
the noise inside the vocabulary head; the per-op loop: inside the argmax kernel).  tau = 0 is the greedy step.  Shapes,
forms, decoders and references are those of the scheduled-sampling tests (test_gpu_sched_sampling.CASES / FORMS /
_decoder / _run), the loss rules those of test_gpu_loss_paths, the end-to-end rules those of test_gpu_shapes,
test_gpu_greedy and test_gpu_feature_grad -- imported, none restated.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from oracle import sat_oracle as O
import loss_reference as R
import sample_host as H
import test_gpu_feature_grad as FG
import test_gpu_greedy as G
import test_gpu_loss_paths as LP
import test_gpu_sched_sampling as SS
import test_gpu_shapes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES, FORMS = SS.CASES, SS.FORMS
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


def _sample_decoder(sat, name, form, train=True):
    c = SS._case(name)
    dtype, step = FORMS[form]
    dec = SS._decoder(sat, c)
    dec = dec.train() if train else dec.eval()
    dec.policy = sat.Policy(greedy_step=step) if step else None
    dec.dropout_mask = c["masks"].permute(1, 0, 2).contiguous().to(torch.uint8)
    return c, dec, dtype


_RUNS = {}


def _run_sample(sat, name, form, tau, tau_dev=False, feats_grad=False, loss="caption", adam=False):
    """SS._run's seeded train-mode step with the forward replaced by Decoder.sample (tau by value, or through the
    device scalar with another value passed by value).  loss: 'caption' (caption_loss on the case's captions, as
    SS._run) or 'weighted' (weighted_caption_loss on the drawn tokens with the case's pseudo-advantages).  Cached."""
    key = (name, form, tau, tau_dev, feats_grad, loss, adam)
    if key in _RUNS:
        return _RUNS[key]
    torch.manual_seed(4321)   # the module's seed comes from torch's generator: the forms of a case share it
    c, dec, dtype = _sample_decoder(sat, name, form)
    B, T1 = c["B"], c["T"] - 1
    opt = sat.Adam(dec.parameters(), lr=S.LR)
    opt.zero_grad()
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).to(dtype).requires_grad_(feats_grad)
    if tau_dev:
        dec.sample_temperature_tensor = torch.tensor([tau], device=DEV, dtype=torch.float32)
    dec._ensure_flat(feats.device)
    noise = dec.sample_noise(B, T1).cpu()          # before the forward: the noise of its counter value
    preds, alphas, sampled = dec.sample(feats, T1, temperature=3.25 if tau_dev else tau)
    assert not sampled.requires_grad and sampled.dtype == torch.int32 and tuple(sampled.shape) == (B, T1)
    h = dict(weights=None)
    if loss == "caption":
        pad, skip = sat.special_ids(c["bert"])
        lo, _ = sat.caption_loss(preds, alphas, caps, 1.0, pad, skip)
    else:
        w = _pseudo_weights(sat, c, sampled)
        lo, logp = sat.weighted_caption_loss(preds, alphas, sampled, w, 1.0)
        h.update(weights=w.cpu(), logp=logp.cpu())
    lo.backward()
    torch.cuda.synchronize()
    params = dict(dec.named_parameters())
    h.update(loss=lo.item(), preds=preds.detach().float().cpu(), alphas=alphas.detach().float().cpu(),
             grads={n: params[n].grad.detach().float().cpu().clone() for n in dec.active_param_names()},
             tokens=dec.last_tokens.long().cpu(), sampled=sampled.long().cpu(), noise=noise,
             feat_grad=None if feats.grad is None else feats.grad.detach().float().cpu(),
             counter=int(dec._seed_dev.item()), seed_host=dec._seed_host)
    if adam:
        opt.step()
        torch.cuda.synchronize()
        h["params"] = {n: params[n].detach().float().cpu().clone() for n in h["grads"]}
    _RUNS[key] = h
    return h


def _pseudo_weights(sat, c, sampled):
    """Fixed pseudo-advantages of mixed sign through scst_weights (the end token of the case's vocabulary)."""
    B = c["B"]
    adv = torch.tensor([0.8, -0.5, 0.3, -0.9][:B], device=sampled.device)
    return sat.scst_weights(sampled, adv, (102,) if c["bert"] else (1,))


def _assert_draw(c, preds, sampled, tokens, noise, tau):
    """sampled = the first-index argmax of preds + tau * noise (two fp32 ops), tokens = the start token then the
    draws"""
    B, T1 = sampled.shape
    scaled = torch.mul(noise.to(DEV), tau)                       # fp32, one rounding
    want = torch.add(preds.to(DEV).float(), scaled).cpu()        # fp32, one rounding
    assert want.dtype == torch.float32
    assert torch.equal(sampled, want.argmax(2))                  # first index on ties, on the CPU
    if tokens is not None:
        assert torch.equal(tokens[:, 0], torch.full_like(tokens[:, 0], SS._start(c)))
        assert torch.equal(tokens[:, 1:], sampled[:, :T1 - 1])


# ------------------------------------------------------------------ 1. tau = 0 is the greedy step
@pytest.mark.parametrize("tau_dev", [False, True], ids=["by_value", "device_scalar"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_zero_temperature_is_the_greedy_step_bit_for_bit(sat, name, form, tau_dev):
    h, g = _run_sample(sat, name, form, 0.0, tau_dev=tau_dev), SS._run(sat, name, form, "greedy")
    assert torch.equal(h["tokens"], g["tokens"])
    assert torch.equal(h["preds"], g["preds"]) and torch.equal(h["alphas"], g["alphas"])
    assert torch.equal(h["sampled"], h["preds"].argmax(2))
    assert h["loss"] == g["loss"]
    assert sorted(h["grads"]) == sorted(g["grads"])
    for n in g["grads"]:
        assert torch.equal(h["grads"][n], g["grads"][n]), n


# ------------------------------------------------------------------ 2. the draw is the stated function
@pytest.mark.parametrize("tau", [1.0, 0.7])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(CASES))
def test_draw_is_the_stated_function(sat, name, form, tau):
    c = SS._case(name)
    h = _run_sample(sat, name, form, tau)
    _assert_draw(c, h["preds"], h["sampled"], h["tokens"], h["noise"], tau)
    assert h["counter"] == 1                                     # advanced once by the forward
    if tau == 1.0:   # the noise moves the choice somewhere (B (T-1) >= 15 draws from a spread-out softmax)
        assert not torch.equal(h["sampled"], h["preds"].argmax(2))


def test_forms_draw_the_same_noise(sat):
    """G depends on (seed, b, t, v) only: the three forms of a case report the same noise for a counter value."""
    for name in ("e128_ado", "e512_simple_l196"):
        n = [_run_sample(sat, name, form, 1.0) for form in FORMS]
        assert n[0]["seed_host"] == n[1]["seed_host"] == n[2]["seed_host"]
        assert torch.equal(n[0]["noise"], n[1]["noise"]) and torch.equal(n[0]["noise"], n[2]["noise"])


# ------------------------------------------------------------------ 3. noise against the host
@pytest.mark.parametrize("shape", [(3, 5, 1003), (1, 1, 30522)], ids=["b3_t5_v1003", "bert_row"])
def test_noise_matches_the_host_restatement(sat, shape):
    """|G_hip - G_fp64| <= 1e-5 max(1, |G|): a sanity check of the formula (two chained fp32 logs accumulate a few ulp;
    the bound is about forty times that)."""
    B, T1, V = shape
    torch.manual_seed(99)
    dec = sat.Decoder(30522 if V == 30522 else V, 512, attention=True)
    dec.vocabulary_size = V
    a = dec.sample_noise(B, T1).cpu()
    b = dec.sample_noise(B, T1).cpu()
    assert torch.equal(a, b)                                      # the same counter: the same values
    ref = H.host_sample_gumbel(H.step_seed(dec._seed_host, 0), B, T1, V)
    err = np.abs(a.double().numpy() - ref) / np.maximum(1.0, np.abs(ref))
    print(f"\n[scst] noise {shape}: worst err / (1e-5 max(1, |G|)) = {err.max() / 1e-5:.4f}", end="")
    assert torch.isfinite(a).all() and err.max() <= 1e-5, err.max()
    dec._seed_dev.fill_(3)                                        # what three forwards leave in the counter
    c = dec.sample_noise(B, T1).cpu()
    assert not torch.equal(c, a)
    ref3 = H.host_sample_gumbel(H.step_seed(dec._seed_host, 3), B, T1, V)
    assert (np.abs(c.double().numpy() - ref3) / np.maximum(1.0, np.abs(ref3))).max() <= 1e-5


def test_noise_differs_after_a_forward_bumped_the_counter(sat):
    c, dec, dtype = _sample_decoder(sat, "e128_ado", "fused")
    B, T1 = c["B"], c["T"] - 1
    feats = c["feats"].to(DEV).to(dtype)
    dec._ensure_flat(feats.device)
    n0 = dec.sample_noise(B, T1)
    with torch.no_grad():
        dec.sample(feats, T1, 1.0)
    n1 = dec.sample_noise(B, T1)
    assert int(dec._seed_dev.item()) == 1 and not torch.equal(n0, n1)
    ref = H.host_sample_gumbel(H.step_seed(dec._seed_host, 1), B, T1, c["V"])
    assert (np.abs(n1.cpu().double().numpy() - ref) / np.maximum(1.0, np.abs(ref))).max() <= 1e-5


# ------------------------------------------------------------------ 4. distribution
DIST = dict(B=128, T1=3, E=128, V=200, D=64, L=16, forwards=40, bins=16, scale=1.0)


@functools.lru_cache(maxsize=None)
def _chi2_upper_quantile(df, q):
    """x with P(chi2(df) > x) = q, by bisection on the regularised upper incomplete gamma function."""
    a = torch.tensor(df / 2.0, dtype=torch.float64)
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if torch.special.gammaincc(a, torch.tensor(mid / 2.0, dtype=torch.float64)).item() > q:
            lo = mid
        else:
            hi = mid
    return hi


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("form", list(FORMS))
def test_draws_follow_the_softmax(sat, form, tau):
    """5120 step-0 draws of one image (eval mode: no dropout, every row shares preds[:, 0]) against
    softmax(preds[0, 0] / tau): Pearson's chi-square over 16 groups of token ids of near-equal expected mass stays under
    the upper 1e-6 quantile of chi2(15).  numpy draws from the oracle's softmax at these parameters stay under it too
    (20 seeds, worst 29.9 at tau = 1 and 29.4 at tau = 0.5 against the bound 56.5)."""
    d = DIST
    torch.manual_seed(1234)
    c = dict(E=d["E"], D=d["D"], V=d["V"], ado=True, att=True, bert=False,
             p=O.make_decoder_params(d["V"], d["D"], d["E"], True, 5, scale=d["scale"]))
    dec = SS._decoder(sat, c).eval()
    dtype, step = FORMS[form]
    dec.policy = sat.Policy(greedy_step=step) if step else None
    one = np.maximum(np.random.default_rng(3).standard_normal((1, d["L"], d["D"])), 0).astype(np.float32)
    feats = torch.from_numpy(one).expand(d["B"], -1, -1).contiguous().to(DEV).to(dtype)
    draws = []
    with torch.no_grad():
        for _ in range(d["forwards"]):
            preds, _, sampled = dec.sample(feats, d["T1"], temperature=tau)
            draws.append(sampled[:, 0])
    torch.cuda.synchronize()
    assert int(dec._seed_dev.item()) == d["forwards"]            # eval mode draws afresh on every call
    x = preds[:, 0].double().cpu()
    assert S.rel(x, x[:1].expand_as(x)) < 1e-2                    # one image: the rows share the step-0 logits
    p = torch.softmax(x[0] / tau, 0).numpy()
    assert p.max() / p.min() >= 3.0                               # visibly non-uniform
    before = np.cumsum(p) - p
    bins = np.minimum(d["bins"] - 1, np.floor(before * d["bins"] + 1e-12).astype(np.int64))
    n = d["B"] * d["forwards"]
    expected = n * np.bincount(bins, weights=p, minlength=d["bins"])
    assert n == 5120 and (expected >= 50).all(), expected
    got = torch.cat(draws).long().cpu().numpy()
    observed = np.bincount(bins[got], minlength=d["bins"])
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    bound = _chi2_upper_quantile(15, 1e-6)
    print(f"\n[scst] distribution {form} tau={tau}: chi2 {chi2:.2f} (bound {bound:.2f}), distinct tokens "
          f"{np.unique(got).size}", end="")
    assert 56.0 < bound < 57.0
    assert chi2 < bound, (chi2, bound)


# ------------------------------------------------------------------ 5. weighted loss
WL = dict(B=3, T=6, L=49, alpha_c=0.37)
W_PATTERN = torch.tensor([[0.50, -0.20, 0.00, 0.30, 0.00],
                          [-0.10, 0.40, 0.25, 0.00, 0.00],
                          [0.35, 0.00, -0.15, 0.20, 0.00]])   # sums to 1.55: the loss does not cancel to nothing
WL_CASES = [(F32, 1003, False), (F32, 2600, False), (F32, 30522, False), (F32, 2600, True),
            (BF16, 1003, False), (BF16, 2600, False), (BF16, 30522, False), (BF16, 1003, True), (BF16, 30522, True)]


def _wl_ids(cases):
    return [f"{LP.NAME[d]}-{v}{'-relu' if r else ''}" for d, v, r in cases]


@functools.lru_cache(maxsize=None)
def _wl_case(dtype, V, relu):
    """Inputs (test_gpu_loss_paths' generator) and the fp64 restatement of the weighted loss, shared and unchanged.
    The last step's weights are zero, so LP.check_grads' rule (the last step exactly zero) applies as it stands."""
    c = R.build_case(WL["B"], WL["T"], V, WL["L"], dtype, "relu" if relu else "randn")
    T1 = WL["T"] - 1
    g = torch.Generator().manual_seed(V + 17)
    targets = torch.randint(0, V, (WL["B"], T1), generator=g, dtype=torch.int32)
    w = W_PATTERN.clone()
    z = c.preds.detach().double().requires_grad_(True)
    a = c.alphas.detach().double().requires_grad_(True)
    x = torch.relu(z) if relu else z
    lse = torch.logsumexp(x, 2)
    xt = x.gather(2, targets.long().unsqueeze(-1)).squeeze(-1)
    ce = (w.double() * (lse - xt)).sum()
    reg = WL["alpha_c"] * ((1.0 - a.sum(1)) ** 2).mean()
    loss = ce + reg
    (LP.G * loss).backward()
    ref = dict(loss=loss.item(), ce=ce.item(), att_reg=reg.item(), logp=(xt - lse).detach(),
               d_preds=z.grad.detach(), d_alphas=a.grad.detach())
    return c, targets, w, ref


def _wl_run(sat, c, targets, w, relu, alpha_c=None):
    p = c.preds.to(DEV).requires_grad_(True)
    a = c.alphas.to(DEV).requires_grad_(True)
    if relu:
        p._sat_relu_logits = True
    seen = {}
    p.register_hook(lambda gr: seen.setdefault("g", gr))
    loss, logp = sat.weighted_caption_loss(p, a, targets.to(DEV), w.to(DEV), WL["alpha_c"] if alpha_c is None else alpha_c)
    assert not logp.requires_grad and logp.dtype == torch.float32
    (LP.G * loss).backward()
    torch.cuda.synchronize()
    return dict(loss=loss.item(), logp=logp.cpu(), hook=seen["g"], d_preds=p.grad.detach().cpu(),
                d_alphas=a.grad.detach().cpu(), bad=loss._sat_bad_targets.cpu())


def _nonzero_rows(t, w):
    """[1, N + 1, V]: the rows of nonzero weight, then one zero row standing where LP.check_grads expects the unscored
    last step"""
    rows = t[w != 0]
    return torch.cat([rows, torch.zeros_like(rows[:1])]).unsqueeze(0)


@pytest.mark.parametrize("dtype,V,relu", WL_CASES, ids=_wl_ids(WL_CASES))
def test_weighted_loss_values_and_gradients(sat, dtype, V, relu):
    c, targets, w, ref = _wl_case(dtype, V, relu)
    out = _wl_run(sat, c, targets, w, relu)
    tag = f"weighted {LP.NAME[dtype]} V={V}{' relu' if relu else ''}"
    # the scalar rule on the loss (the one scalar the entry returns)
    LP.check_scalars(tag, dict(loss=out["loss"], metrics=[out["loss"], out["loss"]]),
                     dict(loss=ref["loss"], ce=ref["loss"], att_reg=ref["loss"]))
    assert float(out["bad"]) == 0.0
    lp_err = ((out["logp"].double() - ref["logp"]).abs() / ref["logp"].abs()).max().item()
    print(f" logp err/bound {lp_err / 1e-4:.4f}", end="")
    assert lp_err <= 1e-4
    # rows of weight zero: exactly zero; the others by the file's rule for the dtype
    zero = out["d_preds"][w == 0]
    assert torch.equal(zero, torch.zeros_like(zero))
    LP.check_grads(tag, dict(d_preds=_nonzero_rows(out["d_preds"], w), d_alphas=out["d_alphas"]),
                   dict(d_preds=_nonzero_rows(ref["d_preds"], w), d_alphas=ref["d_alphas"]), dtype)
    LP.check_padded(tag, out, dtype, V)                           # the padded-ld form and its tag
    assert bool(getattr(out["hook"], "_sat_relu_masked", False)) == relu
    again = _wl_run(sat, c, targets, w, relu)                     # fixed-order reductions: bit-identical
    assert again["loss"] == out["loss"] and torch.equal(again["logp"], out["logp"])
    assert torch.equal(again["d_preds"], out["d_preds"]) and torch.equal(again["d_alphas"], out["d_alphas"])


@pytest.mark.parametrize("dtype,V", [(F32, 1003), (F32, 2600), (BF16, 1003), (BF16, 30522)],
                         ids=["fp32-1003", "fp32-2600", "bf16-1003", "bf16-30522"])
def test_weighted_loss_reduces_to_the_caption_loss(sat, dtype, V):
    """targets = captions[:, 1:], w = 1 / (B (T - 2)) on t < T - 2 and 0 on the last step: the caption loss's own
    reference (LP.case_and_ref) under the same rule."""
    B, T, L = WL["B"], WL["T"], WL["L"]
    c, ref = LP.case_and_ref(dtype, V, "randn", B=B, T=T, L=L)
    w = torch.full((B, T - 1), 1.0 / (B * (T - 2)))
    w[:, -1] = 0.0
    out = _wl_run(sat, c, c.caps[:, 1:].to(torch.int32), w, False, alpha_c=LP.ALPHA_C)
    tag = f"weighted as caption_loss {LP.NAME[dtype]} V={V}"
    LP.check_scalars(tag, dict(loss=out["loss"], metrics=[out["loss"], out["loss"]]),
                     dict(loss=ref["loss"], ce=ref["loss"], att_reg=ref["loss"]))
    LP.check_grads(tag, out, ref, dtype)
    LP.check_padded(tag, out, dtype, V)


def test_out_of_range_targets_count_as_weight_zero(sat):
    """The documented policy: no host read refuses them; the row is scored as weight 0 and tallied."""
    c, targets, w, ref = _wl_case(F32, 1003, False)
    bad_t = targets.clone()
    bad_t[0, 0], bad_t[2, 3] = 1003, -1
    w0 = w.clone()
    w0[0, 0], w0[2, 3] = 0.0, 0.0
    out = _wl_run(sat, c, bad_t, w, False)
    same = _wl_run(sat, c, targets, w0, False)
    assert float(out["bad"]) == 2.0 and float(same["bad"]) == 0.0
    assert out["loss"] == same["loss"] and torch.equal(out["d_preds"], same["d_preds"])
    assert out["logp"][0, 0] == 0 and out["logp"][2, 3] == 0
    z = out["d_preds"][0, 0]
    assert torch.equal(z, torch.zeros_like(z))


# ------------------------------------------------------------------ 6. end to end
def _oracle_weighted(c, h, dtype):
    """S._oracle_fed with the weighted loss written in torch: the oracle teacher-forced on the fed tokens, scoring the
    drawn tokens with the run's weights (alpha_c = 1).  Returns S._oracle_fed's tuple and the feature gradient."""
    p = {k: v.to(dtype) for k, v in c["p"].items()}
    names = O.trainable_names(c["V"], c["D"], c["E"], c["ado"], True, c["bert"])
    q = {k: v.clone().detach().requires_grad_(k in names) for k, v in p.items()}
    T1 = c["T"] - 1
    fed_caps = c["caps"].clone()
    fed_caps[:, :T1] = h["tokens"].to(fed_caps.dtype)
    feats = c["feats"].to(dtype).clone().requires_grad_(True)   # a copy: the case's tensors stay as they are
    preds, alphas, _ = O.decoder_forward(q, feats, fed_caps, tf=True, ado=c["ado"], attention=True, bert=c["bert"],
                                         training=True, dropout_masks=c["masks"].to(dtype))
    lse = torch.logsumexp(preds, 2)
    xt = preds.gather(2, h["sampled"].unsqueeze(-1)).squeeze(-1)
    loss = (h["weights"].to(preds.dtype) * (lse - xt)).sum() + ((1 - alphas.sum(1)) ** 2).mean()
    loss.backward()
    grads = {k: q[k].grad.detach().clone() for k in names if q[k].grad is not None}
    newp = {k: v.detach().clone() for k, v in q.items()}
    O.adam_step(newp, grads, {}, S.LR)
    return (loss.detach(), grads, newp, preds.detach(), alphas.detach()), feats.grad.detach()


def _assert_mixed_sign(h):
    w = h["weights"]
    assert bool((w > 0).any()) and bool((w < 0).any()) and bool((w != 0).all(1).any())


@pytest.mark.parametrize("name", SS.ORACLE_CASES)
def test_end_to_end_fp32_matches_the_fed_token_oracle(sat, name):
    c = SS._case(name)
    fg = name == "e512_ado_v1003"
    h = _run_sample(sat, name, "perop_fp32", 1.0, loss="weighted", feats_grad=fg, adam=True)
    _assert_draw(c, h["preds"], h["sampled"], h["tokens"], h["noise"], 1.0)
    _assert_mixed_sign(h)
    (o32, f32), (o64, f64) = _oracle_weighted(c, h, torch.float32), _oracle_weighted(c, h, torch.float64)
    S._assert_fp32(dict(c, tf=True), h, o32, o64)                # test_gpu_shapes' rule, a reference that feeds tokens
    if fg:
        FG._assert_rule(h["feat_grad"], f32, f64, "sample-mode feature gradient")


@pytest.mark.parametrize("form", ["fused", "perop_bf16"])
@pytest.mark.parametrize("name", SS.ORACLE_CASES)
def test_end_to_end_bf16_matches_the_fed_token_mirror(sat, name, form):
    c = SS._case(name)
    fg = name == "e512_ado_v1003" and form == "fused"
    h = _run_sample(sat, name, form, 1.0, loss="weighted", feats_grad=fg)
    _assert_draw(c, h["preds"], h["sampled"], h["tokens"], h["noise"], 1.0)
    _assert_mixed_sign(h)
    with O.bf16_mirror():
        om, fm = _oracle_weighted(c, h, torch.float64)
    G._assert_mirror(h, om)                                      # test_gpu_greedy's bounds
    if fg:
        err = ((h["feat_grad"] - fm.float()).norm() / fm.float().norm()).item()
        print(f"bf16 sample-mode feature gradient vs the mirror: {err:.3e}")
        assert err <= FG.MIRROR_TOL, err


# ------------------------------------------------------------------ 7. captured graph
def test_captured_step_draws_afresh_and_follows_the_temperature(sat):
    name = "e512_simple_l196"
    c, dec, dtype = _sample_decoder(sat, name, "fused")
    dec.dropout_mask = dec.dropout_mask.to(DEV)
    B, T1 = c["B"], c["T"] - 1
    scalar = torch.tensor([1.0], device=DEV, dtype=torch.float32)
    dec.sample_temperature_tensor = scalar
    feats = c["feats"].to(DEV).to(dtype).detach()   # a leaf without grad: nothing of the backward leaves the device
    assert not feats.requires_grad
    adv = torch.tensor([0.8, -0.5, 0.3, -0.9][:B], device=DEV)
    with torch.no_grad():
        dec.sample(feats, T1, 1.0)   # eager warm-up: draws the host seed, builds the flat buffers
    torch.cuda.synchronize()
    for p in dec.parameters():
        p.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preds, alphas, sampled = dec.sample(feats, T1, 1.0)
        w = sat.scst_weights(sampled, adv, (1,))                  # device-resident weights, recomputed per replay
        loss, logp = sat.weighted_caption_loss(preds, alphas, sampled, w, 1.0)
        loss.backward()
    tokens = dec.last_tokens

    def replay(tau):
        scalar.fill_(tau)
        counter = int(dec._seed_dev.item())
        noise = dec.sample_noise(B, T1).cpu()
        g.replay()
        torch.cuda.synchronize()
        assert int(dec._seed_dev.item()) == counter + 1
        out = (preds.detach().float().cpu(), sampled.long().cpu(), tokens.long().cpu())
        _assert_draw(c, out[0], out[1], out[2], noise, tau)
        assert math.isfinite(loss.item()) and bool(torch.isfinite(dec._grad_flat).all())
        return out

    draws = [replay(1.0)[1] for _ in range(3)]
    assert not torch.equal(draws[0], draws[1]) and not torch.equal(draws[1], draws[2])
    assert not torch.equal(draws[0], draws[2])
    pr, sm, tok = replay(0.0)                                     # the greedy step
    e = SS._run(sat, name, "fused", "greedy")
    assert torch.equal(tok, e["tokens"]) and torch.equal(pr, e["preds"])
    assert torch.equal(sm, pr.argmax(2))


# ------------------------------------------------------------------ 8. learning sanity
LEARN = dict(E=128, D=64, L=16, V=1003, B=64, T=6, steps=60, lr=3e-3)


@pytest.mark.parametrize("form", ["fused", "perop_fp32"])
def test_scst_raises_the_greedy_reward(sat, form):
    """60 SCST steps on fixed features (eval mode: no dropout): a sample, a greedy pass, advantage = r_sample -
    r_greedy, the weighted loss, sat.Adam.  The reward is the fraction of tokens equal to a fixed target sentence: at
    every step the runner-up token of row 0 under the initial model (so the initial greedy reward of that row is 0).
    The mean greedy reward of the last 10 steps must exceed that of the first 10.  The same loop with the oracle on
    the CPU (fp32 torch, these parameters, features, learning rate; torch's generator for the noise) gives
    0.017 -> 0.400 (seed 0) and 0.074 -> 0.400 (seed 1)."""
    d = LEARN
    T1 = d["T"] - 1
    torch.manual_seed(0)
    c = dict(E=d["E"], D=d["D"], V=d["V"], ado=True, att=True, bert=False,
             p=O.make_decoder_params(d["V"], d["D"], d["E"], True, 5))
    dec = SS._decoder(sat, c).eval()
    dtype, step = FORMS[form]
    dec.policy = sat.Policy(greedy_step=step) if step else None
    feats = np.maximum(np.random.default_rng(3).standard_normal((d["B"], d["L"], d["D"])), 0).astype(np.float32)
    feats = torch.from_numpy(feats).to(DEV).to(dtype)
    opt = sat.Adam(dec.parameters(), lr=d["lr"])
    with torch.no_grad():
        p0 = dec.sample(feats, T1, 0.0)[0]
    target = p0[0].float().topk(2, dim=1).indices[:, 1].to(torch.int32)
    greedy_rewards = []
    for _ in range(d["steps"]):
        opt.zero_grad()
        preds, alphas, sampled = dec.sample(feats, T1, 1.0)
        with torch.no_grad():
            greedy = dec.sample(feats, T1, 0.0)[2]
        r_sample = (sampled == target).float().mean(1)
        r_greedy = (greedy == target).float().mean(1)
        w = sat.scst_weights(sampled, r_sample - r_greedy, (1,))
        loss, _ = sat.weighted_caption_loss(preds, alphas, sampled, w, 0.0)
        loss.backward()
        opt.step()
        greedy_rewards.append(r_greedy.mean())
    hist = torch.stack(greedy_rewards).cpu()
    first, last = hist[:10].mean().item(), hist[-10:].mean().item()
    print(f"\n[scst] learning {form}: mean greedy reward {first:.4f} (first 10 steps) -> {last:.4f} (last 10)", end="")
    assert math.isfinite(last) and last > first, (first, last)


# ------------------------------------------------------------------ 9. refusals
def test_refusals(sat):
    name = "e512_ado_v1003"
    c, dec, dtype = _sample_decoder(sat, name, "fused")
    B, T1 = c["B"], c["T"] - 1
    feats = c["feats"].to(DEV).bfloat16()
    for bad in (-0.5, float("nan"), "1.0", True):
        with pytest.raises(ValueError, match="temperature"):
            dec.sample(feats, T1, temperature=bad)
    with pytest.raises(ValueError, match="steps"):
        dec.sample(feats, 1)
    for bad in (torch.ones(1), torch.ones(1, device=DEV, dtype=torch.float64), torch.ones(2, device=DEV)):
        dec.sample_temperature_tensor = bad
        with pytest.raises(ValueError, match="sample_temperature_tensor"):
            dec.sample(feats, T1)
    dec.sample_temperature_tensor = None
    # the C entry refuses teacher-forcing dims and a temperature that is negative or NaN
    L = sat._lib
    caps = c["caps"].to(DEV)
    dec._ensure_flat(feats.device)
    dec._ensure_lp()
    dims = dec._dims(feats, caps)
    lay = dec._layout()
    ws_bytes = L.lib().sat_decoder_workspace_bytes(ctypes.byref(dims))
    ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
    preds = torch.empty(B, T1, c["V"], device=DEV, dtype=torch.bfloat16)
    alphas = torch.empty(B, T1, c["L"], device=DEV, dtype=torch.float32)
    sampled = torch.empty(B, T1, device=DEV, dtype=torch.int32)
    mask = torch.ones(B, T1, c["E"], device=DEV, dtype=torch.uint8)
    dims.has_dropout_mask = 1

    def call(tau, out=sampled):
        return L.lib().sat_decoder_forward_sample(ctypes.byref(dims), ctypes.byref(lay), L.ptr(dec._flat),
                                                  L.ptr(dec._flat_lp), L.ptr(feats), None, L.ptr(mask), tau, None,
                                                  L.ptr(ws), ws_bytes, L.ptr(preds), L.ptr(alphas), None, L.ptr(out),
                                                  L.stream_of(preds))
    dims.tf = 1
    assert call(1.0) == 9001
    dims.tf = 0
    assert call(-0.1) == 9001 and call(float("nan")) == 9001
    assert call(1.0, out=None) == 9001
    assert call(1.0) == 0                                         # captions are not needed
    torch.cuda.synchronize()
    assert bool(((sampled >= 0) & (sampled < c["V"])).all())
    # the loss refuses shapes that do not match
    with pytest.raises(ValueError, match="weighted_caption_loss"):
        sat.weighted_caption_loss(preds, alphas, sampled[:, :-1], torch.zeros(B, T1, device=DEV))
    # eval mode runs without dropout and still draws; use_tf is ignored
    dec.eval()
    dec.use_tf = True
    with torch.no_grad():
        p1, _, s1 = dec.sample(feats, T1, 1.0)
        p2, _, s2 = dec.sample(feats, T1, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(dec.last_tokens[:, 1:], s2[:, :-1])
    assert torch.equal(p1[:, 0], p2[:, 0]) and not torch.equal(s1, s2)


# ------------------------------------------------------------------ 10. the command line
CLI_RUNS = {"cider_bf16": ["--scst-reward", "cider", "--dtype", "bf16"],
            "bleu_fp32": ["--scst-reward", "bleu", "--dtype", "fp32"],
            "cider_bf16_cached": ["--scst-reward", "cider", "--dtype", "bf16", "--cache-features"]}


def _cli(out, extra):
    import json
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(SS.PKG, "train.py"), "--synthetic", "64", "--scst", "--epochs", "1",
                        "--max-steps", "4", "--batch-size", "16", "--log-interval", "1", "--network", "vgg19", "--ado",
                        "--attention", "--vocab", "200", "--seq", "9", "--seed", "7", "--out", str(out)] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "--scst without --model" in r.stderr              # it only warns
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("run", list(CLI_RUNS))
def test_train_cli(sat, tmp_path, run):
    import importlib.util
    import os
    recs = [x for x in _cli(tmp_path, CLI_RUNS[run]) if "scst_reward_sample" in x]
    assert len(recs) == 4
    for x in recs:
        for k in ("scst_reward_sample", "scst_reward_greedy", "scst_logp", "train_loss"):
            assert math.isfinite(x[k]), (k, x)
        assert x["scst_reward_sample"] >= 0 and x["scst_reward_greedy"] >= 0 and x["scst_logp"] < 0
    spec = importlib.util.spec_from_file_location("sat_caption_cli_scst", os.path.join(SS.PKG, "generate_caption.py"))
    gc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gc)
    _, decoder, _, _ = gc.load_model(str(tmp_path / "model_vgg19_1.pth"))
    assert not decoder.training
    if run == "cider_bf16":   # one --seed, two runs: identical checkpoints
        other = tmp_path / "again"
        _cli(other, CLI_RUNS[run])
        a = torch.load(tmp_path / "model_vgg19_1.pth", map_location="cpu", weights_only=True)
        b = torch.load(other / "model_vgg19_1.pth", map_location="cpu", weights_only=True)
        assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)

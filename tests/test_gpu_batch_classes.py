"""The decoder at every batch-size class of its per-step kernels, through the public Decoder module, against the CPU
oracle (fp32 / fp64, and the bf16 rounding mirror in fp64).

B is the dimension a user varies (train.py --batch-size, the ragged last validation batch), and the per-step kernels
pick their code by it: the skinny GEMM's 2 / 4 / 8 row blocks for B <= 32 / 64 / 128 with rows past B clamped on load
and skipped on store; above 128 the tile kernel's partial-output split-K with pick_splits counts, the per-op greedy
step and the skinny vocabulary head; cdiv(256, B) attention-backward chunks per row, ragged over L; the LSTM kernels'
grid cap of 4096 blocks (B E / 64 > 4096: B > 512 at E = 512) with the stride loop behind it; K = B (T - 1) of the
batched products after the loop.  tests/test_cpu_batch_classes.py pins the instance of every case on the host.

D and E decide the skinny eligibility and the LSTM kernels' forms, so they are the production ones; V and T shrink.

  family  D, L, E        V      T  head    feedback  B
  R       2048, 49, 512  1003   4  ado     tf        1, 17, 33, 65, 127, 129     (odd V: padded bf16 head rows)
  V       512, 196, 512  1000   4  simple  tf        1, 33, 129
  G       2048, 49, 512  1003   5  ado     greedy    33, 128, 129
  S       64, 16, 512    120    3  ado     tf        520

Two tests per (family, B, dtype):

a. the whole training step (test_gpu_shapes._hip_step): fp32 by _assert_fp32 unchanged, bf16 against the mirror.
b. isolated rows.  A weight gradient sums over the batch, so one wrong row of 129 moves it by 1 / 129 to 1 / sqrt(129)
   of its norm -- inside every end-to-end bound.  Here the cotangents of preds and alphas are zero outside the rows
   S = {0, 16 floor((B - 1) / 16), B - 1} (the first row, the first row of the last 16-row fragment, the last row), so
   every gradient is the work of the boundary rows alone and a wrong row shows at full scale; and dL/d(features) of
   every other row is a sum of products with a zero cotangent: no nonzero element.

Bounds: fp32 gradients by the project's rule (test_gpu_feature_grad._assert_rule: 2e-4 of the norm, 1e-3 of max|g|,
or twice the oracle's own fp32 / fp64 distance).  bf16 against the mirror: SHAPES_BF16_MIRROR_TOL where the measured
worst is at most two thirds of it, otherwise the measured worst x 1.5, never above BENCH_BF16_MIRROR_TOL; the figures
of every case are in profiles/batch_classes/measured.txt.
"""
import contextlib
import functools

import pytest
import torch

from oracle import sat_oracle as O
import test_gpu_shapes as S
from test_gpu_feature_grad import _assert_rule

pytestmark = pytest.mark.gpu
DEV = "cuda"

# family: (D, L, E, V, T, tf, ado, batch sizes)
FAMILIES = {
    "R": (2048, 49, 512, 1003, 4, True, True, (1, 17, 33, 65, 127, 129)),
    "V": (512, 196, 512, 1000, 4, True, False, (1, 33, 129)),
    "G": (2048, 49, 512, 1003, 5, False, True, (33, 128, 129)),
    "S": (64, 16, 512, 120, 3, True, True, (520,)),
}
# sat_attention_bwd_chunks(B, L, 0) = min(cdiv(256, B), cdiv(L, 4), 16): three chunks over 49 slots (B = 127) is a
# ragged last chunk
CHUNKS = {("R", 1): 13, ("R", 17): 13, ("R", 33): 8, ("R", 65): 4, ("R", 127): 3, ("R", 129): 2,
          ("V", 1): 16, ("V", 33): 8, ("V", 129): 2,
          ("G", 33): 8, ("G", 128): 2, ("G", 129): 2,
          ("S", 520): 1}
# Family G's seeds: on the CPU the fp32 oracle's greedy trajectory keeps at least half of its (row, step) positions
# unambiguous under _greedy_prefix at 1e-5 max|logit| (the cap of _assert_fp32), and the fp64 oracle's ids equal the
# fp32 oracle's on those prefixes, for each of B = 33, 128, 129.
SEEDS = {"R": 201, "V": 211, "G": 223, "S": 227}

CASES = [(f, b, dt) for f, spec in FAMILIES.items() for b in spec[7] for dt in (torch.float32, torch.bfloat16)]
IDS = [f"{f}{b}-{'fp32' if dt == torch.float32 else 'bf16'}" for f, b, dt in CASES]

# bf16 gradient bounds against the mirror, relative error norm per parameter ("feats": dL/d(features) on the rows S),
# from the figures measured on an MI355X (profiles/batch_classes/measured.txt).  A case whose worst parameter is at
# most two thirds of SHAPES_BF16_MIRROR_TOL (1e-2) keeps that bound: test a <= 6.2e-3 (G129), test b <= 3.0e-3 (G128)
# over the cases not listed below.  The listed cases take their measured worst x 1.5, never above
# BENCH_BF16_MIRROR_TOL (2e-2).  What they have in common (measured.txt): 63-100 % of the error norm of f_h.bias or
# f_z.bias sits in one element whose pre-activation in the mirror is 1e-6 .. 9e-5 (standard deviation 0.12-0.23); one
# bf16 rounding of an h / context element falling the other way moves it by 1e-4, the ReLU's derivative flips, and
# every gradient behind that unit carries the one term.  It follows the seed, not the batch class: b G129 (the
# kernels of R129, rows 0 and 128) is at 2.9e-3.
BF16_TOL_DEFAULT = S.SHAPES_BF16_MIRROR_TOL
BF16_TOL_WHOLE = {
    ("R", 127): 1.85e-2,   # measured 1.234e-2 (f_beta.bias)
    ("R", 129): 1.72e-2,   # measured 1.145e-2 (attention.U.weight)
    ("G", 33): 1.45e-2,    # measured 9.637e-3 (f_h.bias)
    ("G", 128): 1.34e-2,   # measured 8.939e-3 (f_beta.bias)
}
BF16_TOL_ROWS = {
    ("R", 129): S.BENCH_BF16_MIRROR_TOL,   # measured 1.512e-2 (f_beta.bias); x 1.5 = 2.27e-2 is above the cap
}


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


@functools.lru_cache(maxsize=None)
def _case(family, B):
    D, Lf, E, V, T, tf, ado, _ = FAMILIES[family]
    return S._make_case(D, Lf, E, V, T, tf, ado, False, B, SEEDS[family] + B)


def _assert_instance(inst, family, B, dtype):
    assert inst["attn_bwd_chunks"] == CHUNKS[family, B], inst
    assert inst["fwd_launches_per_step"] == 4 and inst["bwd_launches_per_step"] == 4, inst
    if dtype == torch.bfloat16:
        assert inst["transposed"] == 1, inst
    else:
        assert (inst["h_splits"], inst["ctx_splits"], inst["dgated_splits"], inst["dh_splits"]) == (1, 1, 1, 1), inst


def _check_bf16(tag, errs, tol):
    print(f"BATCHCLASS {tag}:", " ".join(f"{n}={e:.3e}" for n, e in sorted(errs.items(), key=lambda kv: -kv[1])))
    bad = {n: e for n, e in errs.items() if e >= tol}
    assert not bad, (tol, bad)


# ---------------------------------------------------------------- a. the whole step
@pytest.mark.parametrize("family,B,dtype", CASES, ids=IDS)
def test_whole_step(sat, family, B, dtype):
    c = _case(family, B)
    h = S._hip_step(sat, c, dtype)
    _assert_instance(h["instance"], family, B, dtype)
    if not c["tf"]:   # the fed token of step t is the argmax of step t - 1's stored logits, first index on ties
        assert torch.equal(h["tokens"][:, 1:], h["preds"].argmax(2)[:, :-1])
        assert torch.equal(h["tokens"][:, 0], torch.zeros_like(h["tokens"][:, 0]))
    if dtype == torch.float32:
        S._assert_fp32(c, h, S._oracle(c, torch.float32), S._oracle(c, torch.float64))
        return
    with O.bf16_mirror():
        loss_m, g_m, _, preds_m, alphas_m = S._oracle(c, torch.float64) if c["tf"] else \
            S._oracle_fed(c, h["tokens"], torch.float64)
    e_preds, e_alphas = S.rel(h["preds"], preds_m), S.rel(h["alphas"], alphas_m)
    e_loss = abs(h["loss"] - loss_m.item()) / abs(loss_m.item())
    print(f"BATCHCLASS a {family}{B} bf16 outputs: preds={e_preds:.3e} alphas={e_alphas:.3e} loss={e_loss:.3e}")
    assert sorted(h["grads"]) == sorted(g_m)
    for n, gr in h["grads"].items():
        assert torch.isfinite(gr).all(), n
    errs = S._grad_errors(h, {n: g.float() for n, g in g_m.items()})
    assert e_preds < 1e-2 and e_alphas < 1e-2 and e_loss < 1e-3
    _check_bf16(f"a {family}{B} bf16", errs, BF16_TOL_WHOLE.get((family, B), BF16_TOL_DEFAULT))


# ---------------------------------------------------------------- b. isolated rows
def _rows(B):
    return sorted({0, 16 * ((B - 1) // 16), B - 1})


def _cotangents(c, B):
    """d preds [B, T-1, V] (bf16-representable: the bf16 path takes it without a rounding) and d alphas [B, T-1, L],
    zero outside the rows S."""
    g = torch.Generator().manual_seed(1000 + B)
    T1 = c["T"] - 1
    keep = torch.zeros(B, 1, 1)
    keep[_rows(B)] = 1.0
    Gp = torch.randn(B, T1, c["V"], generator=g).bfloat16().float() * keep
    Ga = torch.randn(B, T1, c["L"], generator=g) * keep
    return Gp, Ga


def _hip_rows(sat, c, dtype, Gp, Ga):
    dec = S._decoder(sat, c).train()
    dec.split_target = 0
    dec.policy = None
    dec.dropout_mask = c["masks"].permute(1, 0, 2).contiguous().to(torch.uint8)
    caps = c["caps"].to(DEV)
    feats = c["feats"].to(DEV).to(dtype).requires_grad_()
    preds, alphas = dec(feats, caps)
    ((preds.float() * Gp.to(DEV)).sum() + (alphas * Ga.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    params = dict(dec.named_parameters())
    grads = {n: params[n].grad.detach().float().cpu().clone() for n in dec.active_param_names()}
    return dict(grads=grads, feats_grad=feats.grad.detach().float().cpu(), tokens=dec.last_tokens.long().cpu(),
                dec=dec, feats=feats, caps=caps, instance=S._instance(sat, dec, feats, caps))


def _oracle_rows(c, dtype, Gp, Ga, fed=None, mirror=False):
    """The oracle's decoder_forward under autograd with the same cotangents; ``fed``: teacher-forced on the tokens the
    HIP decoder fed itself (the argmax feedback is a constant for autograd, as in _oracle_fed)."""
    names = O.trainable_names(c["V"], c["D"], c["E"], c["ado"], True, c["bert"])
    q = {k: v.to(dtype).clone().requires_grad_(k in names) for k, v in c["p"].items()}
    feats = c["feats"].to(dtype).clone().requires_grad_(True)
    caps_in = c["caps"]
    if fed is not None:
        caps_in = c["caps"].clone()
        caps_in[:, :c["T"] - 1] = fed.to(caps_in.dtype)
    with (O.bf16_mirror() if mirror else contextlib.nullcontext()):
        preds, alphas, _ = O.decoder_forward(q, feats, caps_in, tf=True, ado=c["ado"], attention=True, bert=c["bert"],
                                             training=True, dropout_masks=c["masks"].to(dtype))
        ((preds * Gp.to(dtype)).sum() + (alphas * Ga.to(dtype)).sum()).backward()
    grads = {k: q[k].grad.detach() for k in names if q[k].grad is not None}
    return grads, feats.grad.detach()


@pytest.mark.parametrize("family,B,dtype", CASES, ids=IDS)
def test_isolated_rows(sat, family, B, dtype):
    c = _case(family, B)
    rows = _rows(B)
    Gp, Ga = _cotangents(c, B)
    h = _hip_rows(sat, c, dtype, Gp, Ga)
    _assert_instance(h["instance"], family, B, dtype)
    if (family, B, dtype) == ("R", 129, torch.bfloat16):
        # the context product's count: the skinny kernel's at B = 127, pick_splits' at B = 129
        below = S._instance(sat, h["dec"], h["feats"][:127], h["caps"][:127])
        assert below["ctx_splits"] != h["instance"]["ctx_splits"], (below, h["instance"])
    fed = None if c["tf"] else h["tokens"]
    # rows outside S: every term of their dL/d(features) is a product with a zero cotangent
    others = torch.ones(B, dtype=torch.bool)
    others[rows] = False
    stray = (h["feats_grad"][others] != 0).sum().item()   # +-0 compare equal to 0; a NaN does not
    assert stray == 0, (stray, (h["feats_grad"][others] != 0).flatten(1).any(1).nonzero().flatten().tolist()[:8])
    tag = f"b {family}{B} {'fp32' if dtype == torch.float32 else 'bf16'}"
    if dtype == torch.float32:
        g32, f32 = _oracle_rows(c, torch.float32, Gp, Ga, fed)
        g64, f64 = _oracle_rows(c, torch.float64, Gp, Ga, fed)
        assert sorted(h["grads"]) == sorted(g32)
        for n, gr in h["grads"].items():
            if g64[n].norm().item() < 1e-7:
                # attention.v.bias: analytically zero (softmax shift invariance), and so in the fp64 oracle; the
                # fp32 oracle's own value is rounding noise of either sign (1e-7 at these cotangents), so the
                # relative rule has no reference: _assert_fp32's absolute bound for this case
                assert gr.abs().max().item() < 1e-5, n
                continue
            _assert_rule(gr, g32[n], g64[n], f"{tag} {n}")
        _assert_rule(h["feats_grad"][rows], f32[rows], f64[rows], f"{tag} feats")
        return
    g_m, f_m = _oracle_rows(c, torch.float64, Gp, Ga, fed, mirror=True)
    assert sorted(h["grads"]) == sorted(g_m)
    for n, gr in h["grads"].items():
        assert torch.isfinite(gr).all(), n
    errs = S._grad_errors(h, {n: g.float() for n, g in g_m.items()})
    fr = f_m[rows].float()
    errs["feats"] = ((h["feats_grad"][rows] - fr).norm() / fr.norm()).item()
    _check_bf16(tag, errs, BF16_TOL_ROWS.get((family, B), BF16_TOL_DEFAULT))

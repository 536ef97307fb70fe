"""The caption-loss kernels (csrc/loss.hip) on every vocabulary path against the fp64 reference of the whole op
(tests/loss_reference.py): loss, CE, attention regulariser, the four counts, d_preds and d_alphas.

Calls go through the public ``sat_amd.caption_loss`` and autograd, with ``alpha_c = 0.37`` and an upstream factor
``g = 0.75`` so that a factor lost or applied twice shows.  B = 2, T = 4, L = 5 unless stated: six rows, V the only
large dimension.

Which V runs which kernel path (forward ``loss_rows_kernel`` / backward ``loss_bwd_kernel``):

    fp32   V      forward                                               backward
           5      scalar online loop (three waves empty)                scalar
           1003   scalar online loop                                    scalar
           1000   registers, 16-B vectors: one partial chunk            16-B vectors
           1028   registers: the second chunk holds one thread          16-B vectors
           12288  registers, full (the last size that fits)             16-B vectors
           12292  streaming 16-B vectors: the last pass has one thread  16-B vectors
    bf16   7      scalar online loop (odd)                              scalar, rows padded to 8
           1003   scalar online loop (odd)                              scalar, rows padded to 1008
           8      registers, 16-B vectors: one thread                   16-B vectors
           1000   registers: one partial chunk                          16-B vectors
           24576  registers, full (the last size that fits)             16-B vectors
           24584  streaming 16-B vectors (the first size)               16-B vectors
           10     bf16 pairs (the smallest)                             pairs, rows padded to 16
           30522  bf16 pairs (BERT's vocabulary)                        pairs, rows padded to 30528
           32766  bf16 pairs (the last size that fits)                  pairs, rows padded to 32768
           32770  scalar online loop (even, past the pair limit)        pairs, rows padded to 32776

Bounds (each test prints the largest observed ratio to its bound; run with ``-s``):

* scalars (loss, CE, att_reg): |hip - ref| <= 1e-4 |ref|, the project's fp32 parity rule; it holds for bf16 logits
  too, since the reference reads the same rounded logits and the kernel's arithmetic is fp32.
* fp32 d_preds, d_alphas: ||hip - ref|| <= 1e-4 ||ref|| over the tensor and per (b, t) row of d_preds.
* bf16 d_preds: the kernel rounds an fp32 value to bf16 once, to nearest.  bf16 keeps 8 significand bits, so
  neighbours are 2^-7 apart relative to the bottom of their binade and the rounding alone reaches 2^-8 |ref| there
  (2^-9 at the top).  The bound is |hip - ref| <= 2^-8 |ref| + 1e-7 max|ref| per element, no element excepted: at the
  bottom of a binade it leaves the fp32 arithmetic (about 1e-5 relative) only the absolute term's room.  The absolute
  term covers elements whose fp32 value is itself at rounding level.  Measured on an MI355X: the worst element is at
  0.97 of the bound, none over (profiles/loss_paths/tests.log).
* counts, zeros, tags: exact.
"""
import functools
import math

import pytest
import torch

import loss_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALPHA_C, G = 0.37, 0.75
F32, BF16 = torch.float32, torch.bfloat16

V_FP32 = [5, 1003, 1000, 1028, 12288, 12292]
V_BF16 = [7, 1003, 8, 1000, 24576, 24584, 10, 30522, 32766, 32770]
DTYPE_V = [(F32, v) for v in V_FP32] + [(BF16, v) for v in V_BF16]
NAME = {F32: "fp32", BF16: "bf16"}


def _ids(pairs):
    return [f"{NAME[d]}-{v}" for d, v in pairs]


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


@functools.lru_cache(maxsize=None)
def case_and_ref(dtype, V, kind, B=2, T=4, L=5, alpha_c=ALPHA_C, bert=False, variant="scattered", all_pad=False,
                 relu=False):
    """Inputs and their fp64 reference, computed once and shared (never modified) by the tests that need them."""
    c = R.build_case(B, T, V, L, dtype, kind, bert=bert, variant=variant, all_pad=all_pad)
    return c, R.reference_of(c, alpha_c, g=G, relu=relu)


def run_hip(sat, c, alpha_c=ALPHA_C, relu=False, backward=True):
    """caption_loss + (g * loss).backward() on the device; returns host copies and the hooked d_preds itself."""
    p = c.preds.to(DEV).requires_grad_(backward)
    a = c.alphas.to(DEV).requires_grad_(backward)
    if relu:
        p._sat_relu_logits = True
    seen = {}
    if backward:
        p.register_hook(lambda gr: seen.setdefault("g", gr))
    loss, metrics = sat.caption_loss(p, a, c.caps.to(DEV), alpha_c, c.pad_id, c.skip_ids)
    out = dict(loss_t=loss, metrics_t=metrics)
    if backward:
        (G * loss).backward()
        out.update(hook=seen["g"], d_preds=p.grad.detach().cpu(), d_alphas=a.grad.detach().cpu())
    torch.cuda.synchronize()
    out.update(loss=loss.item(), metrics=metrics.detach().cpu().tolist())
    return out


def check_scalars(tag, out, ref):
    """loss / CE / att_reg within 1e-4 relative; returns the ratios to the bound."""
    ratios = {}
    for name, got, want in (("loss", out["loss"], ref["loss"]), ("ce", out["metrics"][0], ref["ce"]),
                            ("att_reg", out["metrics"][1], ref["att_reg"])):
        assert math.isfinite(got), (tag, name, got)
        bound = 1e-4 * abs(want)
        err = abs(got - want)
        ratios[name] = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    print(f"\n[loss_paths] {tag}: scalars err/bound " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()), end="")
    assert all(r <= 1.0 for r in ratios.values()), (tag, ratios, out["loss"], ref["loss"])
    return ratios


def check_counts(tag, out, ref):
    got = [out["metrics"][i] for i in (2, 3, 4, 5)]
    want = [float(ref[k]) for k in ("n_top1", "n_top5", "n_nonpad", "caption_length")]
    assert got == want, (tag, "n_top1 n_top5 n_nonpad caption_length", got, want)


def check_grads(tag, out, ref, dtype, also_zero=None):
    """d_preds / d_alphas against fp64 by the module's bounds; the unscored last step exactly zero."""
    dp, da = out["d_preds"].double(), out["d_alphas"].double()
    rp, ra = ref["d_preds"], ref["d_alphas"]
    assert dp.shape == rp.shape and da.shape == ra.shape
    assert torch.isfinite(dp).all() and torch.isfinite(da).all(), tag
    assert torch.equal(dp[:, -1], torch.zeros_like(dp[:, -1])), (tag, "last step scored")
    if also_zero is not None:
        assert (dp[also_zero] == 0).all(), (tag, "nonzero gradient at a -inf logit")
    ra_n = ra.norm().item()
    r_da = ((da - ra).norm().item() / (1e-4 * ra_n)) if ra_n > 0 else (0.0 if da.abs().max().item() == 0 else math.inf)
    if dtype == F32:
        r_all = (dp - rp).norm().item() / (1e-4 * rp.norm().item())
        rows_ref = rp[:, :-1].flatten(0, 1).norm(dim=1)
        r_row = ((dp - rp)[:, :-1].flatten(0, 1).norm(dim=1) / (1e-4 * rows_ref)).max().item()
        print(f"\n[loss_paths] {tag}: grads err/bound d_preds {r_all:.4f} worst row {r_row:.4f} d_alphas {r_da:.4f}",
              end="")
        assert r_all <= 1.0 and r_row <= 1.0 and r_da <= 1.0, (tag, r_all, r_row, r_da)
    else:
        bound = 2.0 ** -8 * rp.abs() + 1e-7 * rp.abs().max()
        ratio = ((dp - rp).abs() / bound)
        worst, n_bad = ratio.max().item(), int((ratio > 1.0).sum())
        print(f"\n[loss_paths] {tag}: grads err/bound d_preds worst element {worst:.4f} ({n_bad} over) "
              f"d_alphas {r_da:.4f}", end="")
        assert n_bad == 0 and r_da <= 1.0, (tag, worst, n_bad, r_da)


def check_padded(tag, out, dtype, V):
    """bf16 rows that are no multiple of 8: the hooked gradient is the tagged [..., :V] view of rows padded to ld,
    whose pad columns (read through the storage) are exactly zero."""
    gr = out["hook"]
    B, T1, _ = gr.shape
    if dtype == BF16 and V % 8:
        ld = (V + 7) // 8 * 8
        assert getattr(gr, "_sat_padded_ld", None) == ld, tag
        assert gr.stride() == (T1 * ld, ld, 1), (tag, gr.stride())
        full = torch.as_strided(gr, (B, T1, ld), (T1 * ld, ld, 1), gr.storage_offset())
        assert torch.equal(full[..., :V], gr)
        pad = full[..., V:]
        assert torch.equal(pad, torch.zeros_like(pad)), (tag, "pad columns not zero")
    else:
        assert not hasattr(gr, "_sat_padded_ld"), tag
        assert gr.is_contiguous()


# ---------------------------------------------------------------------------- forward, every path
@pytest.mark.parametrize("kind", ["randn", "wide", "shifted"])
@pytest.mark.parametrize("dtype,V", DTYPE_V, ids=_ids(DTYPE_V))
def test_forward_every_path(sat, dtype, V, kind):
    c, ref = case_and_ref(dtype, V, kind)
    out = run_hip(sat, c, backward=False)
    tag = f"forward {NAME[dtype]} V={V} {kind}"
    check_scalars(tag, out, ref)
    check_counts(tag, out, ref)


@pytest.mark.parametrize("dtype,V", DTYPE_V, ids=_ids(DTYPE_V))
def test_ties_rank(sat, dtype, V):
    """Equal logits: the target is ranked behind equal logits of a lower index only (B = 5: fifteen rows, every
    planted situation three times)."""
    B, T = 5, 4
    c, ref = case_and_ref(dtype, V, "ties", B=B)
    assert torch.equal(ref["rank"], c.planted_rank)
    out = run_hip(sat, c, backward=False)
    tag = f"ties {NAME[dtype]} V={V}"
    check_counts(tag, out, ref)
    n_top1, n_top5, n_nonpad = out["metrics"][2:5]
    # the hand-derived table: ranks 0, 1, 4, 5, 5, each on three rows (V = 5 holds only ranks 0 and 1)
    want = (3.0, 9.0) if V >= 7 else (float((c.planted_rank == 0).sum()), 15.0)
    assert (n_top1, n_top5, n_nonpad) == (*want, 15.0), (tag, n_top1, n_top5, n_nonpad)
    check_scalars(tag, out, ref)


# ---------------------------------------------------------------------------- backward, every path
@pytest.mark.parametrize("kind", ["randn", "wide"])
@pytest.mark.parametrize("dtype,V", DTYPE_V, ids=_ids(DTYPE_V))
def test_backward_every_path(sat, dtype, V, kind):
    c, ref = case_and_ref(dtype, V, kind)
    out = run_hip(sat, c)
    tag = f"backward {NAME[dtype]} V={V} {kind}"
    check_grads(tag, out, ref, dtype)
    check_padded(tag, out, dtype, V)


RELU_CASES = [(F32, 12292), (BF16, 1000), (BF16, 30522), (BF16, 1003)]


@pytest.mark.parametrize("dtype,V", RELU_CASES, ids=_ids(RELU_CASES))
def test_backward_relu_mask(sat, dtype, V):
    """ReLU'd logits tagged ``_sat_relu_logits``: the gradient with respect to the ReLU's input."""
    c, ref = case_and_ref(dtype, V, "relu", relu=True)
    assert (c.preds == 0).any()
    out = run_hip(sat, c, relu=True)
    tag = f"relu {NAME[dtype]} V={V}"
    check_scalars(tag, out, ref)
    check_counts(tag, out, ref)                 # relu(randn) is half zeros: exact ties at every rank
    check_grads(tag, out, ref, dtype, also_zero=(c.preds <= 0))
    check_padded(tag, out, dtype, V)
    assert getattr(out["hook"], "_sat_relu_masked", False)


# ---------------------------------------------------------------------------- shape edges
EDGE_V = [(F32, 1003), (BF16, 30522)]


def _full(sat, tag, dtype, V, **kw):
    c, ref = case_and_ref(dtype, V, "randn", **kw)
    out = run_hip(sat, c, alpha_c=kw.get("alpha_c", ALPHA_C))
    check_scalars(tag, out, ref)
    check_counts(tag, out, ref)
    check_grads(tag, out, ref, dtype)
    check_padded(tag, out, dtype, V)
    return c, ref, out


@pytest.mark.parametrize("dtype,V", EDGE_V, ids=_ids(EDGE_V))
def test_smallest_call(sat, dtype, V):
    _full(sat, f"B=1 T=3 L=1 {NAME[dtype]} V={V}", dtype, V, B=1, T=3, L=1)


@pytest.mark.parametrize("dtype,V", EDGE_V, ids=_ids(EDGE_V))
def test_ragged_regulariser_blocks(sat, dtype, V):
    """B * L = 588: three blocks of loss_reg_kernel, the last one ragged."""
    _full(sat, f"B=3 T=6 L=196 {NAME[dtype]} V={V}", dtype, V, B=3, T=6, L=196)


@pytest.mark.parametrize("dtype,V", EDGE_V, ids=_ids(EDGE_V))
def test_alpha_c_zero(sat, dtype, V):
    c, ref, out = _full(sat, f"alpha_c=0 {NAME[dtype]} V={V}", dtype, V, alpha_c=0.0)
    assert out["metrics"][1] == 0.0
    assert torch.equal(out["d_alphas"], torch.zeros_like(out["d_alphas"]))
    assert out["loss"] == out["metrics"][0]


@pytest.mark.parametrize("dtype,V", EDGE_V, ids=_ids(EDGE_V))
def test_bert_ids(sat, dtype, V):
    c, ref, out = _full(sat, f"bert ids {NAME[dtype]} V={V}", dtype, V, bert=True)
    assert (c.pad_id, c.skip_ids) == sat.special_ids(True)


@pytest.mark.parametrize("dtype,V", EDGE_V, ids=_ids(EDGE_V))
def test_all_pad_batch(sat, dtype, V):
    c, ref, out = _full(sat, f"all pad {NAME[dtype]} V={V}", dtype, V, all_pad=True)
    assert out["metrics"][2:6] == [0.0, 0.0, 0.0, 0.0]
    vals = sat.StepMetrics(out["loss_t"], out["metrics_t"]).values()
    assert vals["acc1"] == 0 and vals["acc5"] == 0 and vals["caption_length"] == 0
    assert math.isfinite(vals["loss"])


# ---------------------------------------------------------------------------- -inf logits
NEG_INF = [(F32, 1003), (F32, 12292), (BF16, 1003), (BF16, 24584),     # the online paths
           (F32, 1000), (BF16, 30522)]                                 # registers and pairs, as controls


@pytest.mark.parametrize("variant", ["scattered", "block"])
@pytest.mark.parametrize("dtype,V", NEG_INF, ids=_ids(NEG_INF))
def test_neg_inf_logits(sat, dtype, V, variant):
    """-inf at non-target positions (a masked part of the vocabulary): a finite loss, zero gradient there."""
    c, ref = case_and_ref(dtype, V, "neg_inf", variant=variant)
    out = run_hip(sat, c)
    tag = f"neg_inf/{variant} {NAME[dtype]} V={V}"
    check_scalars(tag, out, ref)
    check_counts(tag, out, ref)
    check_grads(tag, out, ref, dtype, also_zero=c.neg_inf_mask)
    check_padded(tag, out, dtype, V)


# ---------------------------------------------------------------------------- run to run
ONE_PER_PATH = [(F32, 1003), (F32, 1000), (F32, 12292), (BF16, 1003), (BF16, 1000), (BF16, 24584), (BF16, 30522)]


@pytest.mark.parametrize("dtype,V", ONE_PER_PATH, ids=_ids(ONE_PER_PATH))
def test_run_to_run_bit_identical(sat, dtype, V):
    """The kernels sum in a fixed order (loss.hip's header): two runs on the same inputs agree bit for bit."""
    c, _ = case_and_ref(dtype, V, "randn")
    a, b = run_hip(sat, c), run_hip(sat, c)
    assert torch.equal(a["loss_t"], b["loss_t"]) and torch.equal(a["metrics_t"], b["metrics_t"])
    assert torch.equal(a["d_preds"], b["d_preds"]) and torch.equal(a["d_alphas"], b["d_alphas"])

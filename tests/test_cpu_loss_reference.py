"""The fp64 caption-loss reference (tests/loss_reference.py) against the oracle, before the HIP kernels are judged
by it (tests/test_gpu_loss_paths.py): loss, accuracies and caption length on tie-free inputs with both special-id
sets, the hand-derived ranks of the planted ties, -inf logits against F.cross_entropy, the all-pad batch, and the
builder's determinism."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_reference as R
from oracle import sat_oracle as O

ALPHA_C = 0.37


@pytest.mark.parametrize("kind", ["randn", "wide", "shifted"])
@pytest.mark.parametrize("B,T,V,L,bert", [(2, 4, 1003, 5, False), (2, 4, 1003, 5, True), (3, 6, 1200, 7, False),
                                          (3, 6, 1200, 7, True), (1, 3, 5, 1, False)])
def test_reference_matches_oracle(B, T, V, L, bert, kind):
    c = R.build_case(B, T, V, L, torch.float32, kind, seed=3, bert=bert)
    ref = R.reference_of(c, ALPHA_C)
    x = c.preds.double()
    want = O.caption_loss(x, c.alphas.double(), c.caps, ALPHA_C).item()
    assert abs(ref["loss"] - want) <= 1e-12 * abs(want)
    assert abs(ref["ce"] + ref["att_reg"] - ref["loss"]) <= 1e-12 * abs(want)
    targets = c.caps[:, 1:]
    assert ref["n_nonpad"] == int((targets != c.pad_id).sum())
    assert ref["caption_length"] == O.calculate_caption_lengths(c.caps, c.skip_ids)
    # the accuracies on tie-free rows only: top-k's choice among equal logits is not defined (randn + 100 in fp32
    # repeats values; randn and randn * 30 do not)
    tie_free = all(len(torch.unique(row)) == V for row in x.reshape(-1, V))
    assert tie_free or kind == "shifted"
    if not tie_free:
        return
    for k, key in ((1, "n_top1"), (5, "n_top5")):
        acc = O.sequence_accuracy(x, targets, k, c.pad_id)
        assert ref["n_nonpad"] > 0
        assert abs(100.0 * ref[key] / ref["n_nonpad"] - acc) < 1e-9


def test_reference_gradients_scale_and_alpha_c():
    """d_preds / d_alphas are the gradients of g * loss: against the oracle's autograd, with g and alpha_c that a lost
    or doubled factor would show in."""
    c = R.build_case(2, 5, 60, 6, torch.float32, "randn", seed=1)
    g = 0.75
    ref = R.reference_of(c, ALPHA_C, g=g)
    p = c.preds.double().requires_grad_(True)
    a = c.alphas.double().requires_grad_(True)
    (g * O.caption_loss(p, a, c.caps, ALPHA_C)).backward()
    assert torch.allclose(ref["d_preds"], p.grad, rtol=1e-12, atol=1e-18)
    assert torch.allclose(ref["d_alphas"], a.grad, rtol=1e-12, atol=1e-18)
    assert torch.equal(ref["d_preds"][:, -1], torch.zeros_like(ref["d_preds"][:, -1]))   # the unscored last step
    # through the ReLU: the gradient with respect to z, zero where z <= 0
    c = R.build_case(2, 5, 60, 6, torch.float32, "randn", seed=2)
    ref = R.reference_of(c, ALPHA_C, g=g, relu=True)
    z = c.preds.double().requires_grad_(True)
    (g * O.caption_loss(torch.relu(z), c.alphas.double(), c.caps, ALPHA_C)).backward()
    assert torch.allclose(ref["d_preds"], z.grad, rtol=1e-12, atol=1e-18)
    assert (ref["d_preds"][c.preds <= 0] == 0).all() and (c.preds <= 0).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [5, 7, 8, 10, 1000, 1003, 1028, 12292, 32770])
def test_ties_counts_hand_derived(V, dtype):
    B, T = 5, 4
    c = R.build_case(B, T, V, 5, dtype, "ties")
    ref = R.reference_of(c, ALPHA_C)
    assert torch.equal(c.preds.float().to(dtype), c.preds)      # every value exact in bf16
    assert torch.equal(ref["rank"], c.planted_rank)
    assert bool(ref["nonpad"].all()) and ref["n_nonpad"] == B * (T - 1)
    if V >= 7:
        # every situation on three of the fifteen rows: ranks 0, 1, 4, 5, 5
        assert sorted(c.planted_rank.flatten().tolist()) == [0] * 3 + [1] * 3 + [4] * 3 + [5] * 6
        assert (ref["n_top1"], ref["n_top5"]) == (3, 9)
    else:
        # V = 5 holds only (0,0,3) and (0,1,0); every rank is below 5
        assert set(c.planted_rank.flatten().tolist()) == {0, 1}
        assert ref["n_top1"] == int((c.planted_rank == 0).sum()) and ref["n_top5"] == B * (T - 1)
    # the planted targets include both ends of the row
    tg = c.caps[:, 1:]
    assert (tg == 0).any() and (tg == V - 1).any()
    # each situation as planted: count it straight from the row
    x = c.preds.double()
    for b in range(B):
        for t in range(T - 1):
            row, k = x[b, t], int(tg[b, t])
            n_gt, n_before, n_after = int((row > row[k]).sum()), int((row[:k] == row[k]).sum()), int((row[k + 1:] == row[k]).sum())
            assert ((n_gt, n_before, n_after), n_gt + n_before) in R.TIE_SITUATIONS
            assert n_gt + n_before == int(c.planted_rank[b, t])


@pytest.mark.parametrize("variant", ["scattered", "block"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [1003, 12292])
def test_neg_inf_finite_and_equals_cross_entropy(V, dtype, variant):
    B, T, L = 2, 4, 5
    c = R.build_case(B, T, V, L, dtype, "neg_inf", variant=variant)
    m = c.neg_inf_mask
    assert m.any() and torch.equal(torch.isinf(c.preds), m)
    assert not m.gather(2, c.caps[:, 1:].unsqueeze(-1)).any()   # targets are finite
    if variant == "block":
        assert m[..., 1:min(1000, V // 2)].float().mean() > 0.99
    ref = R.reference_of(c, ALPHA_C, g=0.75)
    assert math.isfinite(ref["loss"])
    assert torch.isfinite(ref["d_preds"]).all() and torch.isfinite(ref["d_alphas"]).all()
    assert (ref["d_preds"][m] == 0).all()
    p = c.preds.double().requires_grad_(True)
    Tl = T - 2
    ce = F.cross_entropy(p[:, :Tl].transpose(0, 1).reshape(-1, V), c.caps[:, 1:1 + Tl].transpose(0, 1).reshape(-1))
    (0.75 * ce).backward()
    assert abs(ref["ce"] - ce.item()) <= 1e-12 * abs(ce.item())
    assert torch.allclose(ref["d_preds"], p.grad, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("bert", [False, True], ids=["plain", "bert"])
def test_all_pad_batch(bert):
    c = R.build_case(2, 4, 1003, 5, torch.float32, "randn", bert=bert, all_pad=True)
    ref = R.reference_of(c, ALPHA_C)
    assert (ref["n_nonpad"], ref["n_top1"], ref["n_top5"], ref["caption_length"]) == (0, 0, 0, 0)
    assert math.isfinite(ref["loss"])                                 # pads are scored all the same
    assert O.sequence_accuracy(c.preds.double(), c.caps[:, 1:], 1, c.pad_id) == 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_builder_is_deterministic(kind):
    a = R.build_case(5, 4, 1003, 5, torch.bfloat16, kind, seed=4)
    b = R.build_case(5, 4, 1003, 5, torch.bfloat16, kind, seed=4)
    assert torch.equal(a.preds.float().nan_to_num(neginf=-1e30), b.preds.float().nan_to_num(neginf=-1e30))
    assert torch.equal(a.alphas, b.alphas) and torch.equal(a.caps, b.caps)
    other = R.build_case(5, 4, 1003, 5, torch.bfloat16, kind, seed=5)
    assert not torch.equal(a.preds.float().nan_to_num(neginf=-1e30), other.preds.float().nan_to_num(neginf=-1e30))
    assert a.preds.dtype == torch.bfloat16 and a.alphas.dtype == torch.float32 and a.caps.dtype == torch.int64

"""fp64 reference of the whole caption-loss op, and a seeded builder of its inputs.

A plain helper module (no fixtures, no GPU): ``tests/test_cpu_loss_reference.py`` checks it against the oracle,
``tests/test_gpu_loss_paths.py`` judges the HIP kernels by it.

The reference is computed from the values the kernel actually reads: ``preds`` in their own dtype (bf16 inputs are
rounded to bf16 by the builder, so nothing is rounded here) and ``alphas`` in fp32, both taken to fp64.

    ce       = mean_{t < T-2, b} (logsumexp(x[b,t]) - x[b,t,tgt])        tgt = captions[b, t+1]; pads included
    att_reg  = alpha_c * mean_{b,l} (1 - sum_t alphas[b,t,l])^2
    loss     = ce + att_reg
    C[b,t]   = #{v : x[v] > x[tgt]} + #{v < tgt : x[v] == x[tgt]}        all T-1 steps (rank of the target; ties
                                                                         go to the lower index, as in topk)
    n_top1   = sum [tgt != pad and C < 1],  n_top5 = sum [tgt != pad and C < 5],  n_nonpad = sum [tgt != pad]
    caption_length = number of caption tokens not in skip_ids
    d_preds, d_alphas = fp64 autograd of g * loss (through relu(z) with respect to z for the ReLU variant)
"""
from dataclasses import dataclass

import numpy as np
import torch

from oracle import sat_oracle as O

PLAIN = (3, (3, 0, 1))         # pad_id, skip_ids (pad, start, eos)
BERT = (0, (0, 101, 102))

KINDS = ("randn", "wide", "shifted", "relu", "ties", "neg_inf")

# (n_gt, n_before, n_after) -> rank C of the target: n_gt + n_before
TIE_SITUATIONS = (((0, 0, 3), 0), ((0, 1, 0), 1), ((4, 0, 2), 4), ((4, 1, 0), 5), ((5, 0, 0), 5))


@dataclass
class Case:
    preds: torch.Tensor            # [B, T-1, V] in the kernel's dtype
    alphas: torch.Tensor           # [B, T-1, L] fp32
    caps: torch.Tensor             # [B, T] int64
    pad_id: int
    skip_ids: tuple
    planted_rank: torch.Tensor = None      # ties: the hand-derived rank of every (b, t)
    neg_inf_mask: torch.Tensor = None      # neg_inf: where the -inf logits are


def all_pad_captions(B, T, bert=False):
    """<start> followed by pads only: every target is the pad token."""
    pad_id, _ = BERT if bert else PLAIN
    start = O.SPECIAL_BERT["start"] if bert else O.SPECIAL_PLAIN["start"]
    caps = torch.full((B, T), pad_id, dtype=torch.int64)
    caps[:, 0] = start
    return caps


def _spread(lo, hi, n, from_top=False):
    """n distinct integers of [lo, hi), evenly spread, both ends included for n >= 2 (the low end for n == 1, the
    high end with from_top)."""
    if n == 0:
        return []
    assert hi - lo >= n
    if n == 1:
        return [hi - 1 if from_top else lo]
    out = sorted(set(int(round(v)) for v in np.linspace(lo, hi - 1, n)))
    assert len(out) == n
    return out


def _plant_ties(x, V, pad_id):
    """Overwrite every row of x [B, T-1, V] (background strictly below 0) with one rank situation and return
    (targets [B, T-1], ranks [B, T-1]).  Row i = b * (T-1) + t gets situation (b + t) % 5 -- the next one that fits
    where V is too small for it (a situation needs n_gt + n_before + n_after + 1 logits)."""
    B, T1, _ = x.shape
    tgts = torch.zeros(B, T1, dtype=torch.int64)
    ranks = torch.zeros(B, T1, dtype=torch.int64)
    fits = [s for s in TIE_SITUATIONS if sum(s[0]) + 1 <= V]
    assert fits
    for b in range(B):
        for t in range(T1):
            want = TIE_SITUATIONS[(b + t) % 5]
            (n_gt, n_before, n_after), rank = want if want in fits else fits[(b + t) % len(fits)]
            i = b * T1 + t
            # the target: the two ends of the row first (V-1 lies in the last, partial, vector), then the inside
            cands = [0, V - 1, V // 2, (3 * V) // 4, V // 3, 1, V - 2]
            cands = cands[i % 5:] + cands[:i % 5] + list(range(V))
            tgt = next(c for c in cands
                       if 0 <= c < V and c != pad_id and c >= n_before and V - 1 - c >= n_after)
            before = _spread(0, tgt, n_before)                      # n = 1: index 0
            after = _spread(tgt + 1, V, n_after, from_top=True)     # n = 1: index V-1
            taken = set(before) | set(after) | {tgt}
            free = [v for v in range(V) if v not in taken] if V <= 64 else None
            if free is None:
                # spread over the whole row (different lanes, threads, waves and register chunks), both ends if free
                free = [v for v in _spread(0, V, min(V, 4 * n_gt + 16)) if v not in taken]
            greater = [free[k] for k in _spread(0, len(free), n_gt)]
            x[b, t, tgt] = 0.0
            for v in before + after:
                x[b, t, v] = 0.0
            for j, v in enumerate(greater):
                x[b, t, v] = float(j + 1)
            tgts[b, t], ranks[b, t] = tgt, rank
    return tgts, ranks


def build_case(B, T, V, L, dtype, kind, seed=0, bert=False, variant="scattered", all_pad=False):
    """Deterministic inputs of one caption_loss call.  kind: see KINDS; variant: the neg_inf layout ('scattered':
    -inf at about one non-target position in eight; 'block': -inf over the whole index range [1, min(1000, V/2)),
    targets excepted)."""
    assert kind in KINDS and dtype in (torch.float32, torch.bfloat16)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * KINDS.index(kind) + V)
    pad_id, skip_ids = BERT if bert else PLAIN
    T1 = T - 1
    x = torch.randn(B, T1, V, generator=g)
    alphas = torch.softmax(torch.randn(B, T1, L, generator=g), -1)
    if all_pad:
        caps = all_pad_captions(B, T, bert)
    else:
        caps = O.make_captions(B, T, V, seed + 1, bert=bert)
    case = Case(None, alphas, caps, pad_id, skip_ids)
    if kind == "wide":
        x = x * 30.0
    elif kind == "shifted":
        x = x + 100.0
    elif kind == "relu":
        x = torch.relu(x)
    elif kind == "ties":
        x = (0.5 * x - 5.0).clamp_(max=-1.0).bfloat16().float()     # exact in bf16, strictly below the target's 0
        tgts, ranks = _plant_ties(x, V, pad_id)
        caps = caps.clone()
        caps[:, 1:] = tgts
        case.caps, case.planted_rank = caps, ranks
    elif kind == "neg_inf":
        if variant == "scattered":
            mask = torch.rand(B, T1, V, generator=g) < 0.125
        else:
            assert variant == "block"
            mask = torch.zeros(B, T1, V, dtype=torch.bool)
            mask[..., 1:min(1000, V // 2)] = True
        mask.scatter_(2, case.caps[:, 1:].unsqueeze(-1), False)      # targets are always finite
        x = x.masked_fill(mask, float("-inf"))
        case.neg_inf_mask = mask
    case.preds = x.to(dtype)
    return case


def reference(preds, alphas, caps, alpha_c, pad_id, skip_ids, g=1.0, relu=False):
    """The whole op in fp64 (module docstring).  Returns a dict of python numbers and fp64 tensors."""
    B, T1, V = preds.shape
    z = preds.detach().double().requires_grad_(True)
    a = alphas.detach().float().double().requires_grad_(True)
    x = torch.relu(z) if relu else z
    tg = caps[:, 1:].long()
    xt = x.gather(2, tg.unsqueeze(-1)).squeeze(-1)                   # [B, T1]
    lse = torch.logsumexp(x, dim=2)
    Tl = T1 - 1
    ce = (lse - xt)[:, :Tl].sum() / (B * Tl)
    att_reg = alpha_c * ((1.0 - a.sum(1)) ** 2).mean()
    loss = ce + att_reg
    (g * loss).backward()
    loss, ce, att_reg = loss.detach(), ce.detach(), att_reg.detach()
    with torch.no_grad():
        idx = torch.arange(V).view(1, 1, V)
        rank = (x > xt.unsqueeze(-1)).sum(-1) + ((x == xt.unsqueeze(-1)) & (idx < tg.unsqueeze(-1))).sum(-1)
        nonpad = tg != pad_id
        skip = torch.as_tensor(list(skip_ids))
        cap_len = int((~(caps.unsqueeze(-1) == skip).any(-1)).sum())
    return dict(loss=loss.item(), ce=ce.item(), att_reg=att_reg.item(),
                rank=rank, nonpad=nonpad,
                n_top1=int((nonpad & (rank < 1)).sum()), n_top5=int((nonpad & (rank < 5)).sum()),
                n_nonpad=int(nonpad.sum()), caption_length=cap_len,
                d_preds=z.grad.detach(), d_alphas=a.grad.detach() if a.grad is not None else torch.zeros_like(a))


def reference_of(case, alpha_c, g=1.0, relu=False):
    return reference(case.preds, case.alphas, case.caps, alpha_c, case.pad_id, case.skip_ids, g=g, relu=relu)

"""What self-critical sequence training costs on the device, bf16, training mode, at the cfg4 shape -- B 128, L 49,
D 2048, E 512, V 10000, T 27, ado + attention -- forms replayed in turn in one process:

    greedy_fwd      the greedy forward alone (tf=False, the fused greedy step): the yardstick of the sample forward
    sample_fwd      Decoder.sample at temperature 1 alone
    sample_fwd_t0   Decoder.sample at temperature 0 (the greedy tokens through the sample instances)
    greedy_step     greedy forward + caption_loss + backward (the existing step; it must not move)
    sample_step     sample forward + weighted_caption_loss (device-resident weights) + backward
    loss_caption    caption_loss forward + backward on fixed logits
    loss_weighted   weighted_caption_loss forward + backward on the same logits

and the whole eager SCST step from cached features (two forwards, the host reward, the loss, the backward, Adam) with
the host reward's share, for CIDEr-D and sentence BLEU-4 on synthetic references.

    python tools/scst_bench.py [--batch 128] [--repeats 9] [--replays 100] [--steps 20] [--out FILE]

Each repeat times --replays replays of every captured form between device events, the forms alternating; the result is
the median ms per replay over the repeats with min..max.  Writes profiles/scst/step_times.json and prints it as one
JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import sat_amd  # noqa: E402
from sat_amd import bleu as bleu_mod  # noqa: E402
from sat_amd import cider as cider_mod  # noqa: E402
from sat_amd.data import synthetic_captions  # noqa: E402

L, D, V, T = 49, 2048, 10000, 27


def decoder(dev):
    torch.manual_seed(0)
    dec = sat_amd.Decoder(V, D, tf=False, ado=True, attention=True).to(dev).train()
    dec.record_tokens = False
    return dec


def capture(step):
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    return graph, out


def build(B, dev):
    feats = torch.randn(B, L, D, device=dev).relu().bfloat16()
    caps = synthetic_captions(B, T, V, generator=torch.Generator().manual_seed(1), device=dev)
    pad, skip = sat_amd.special_ids(False)
    adv = torch.linspace(-1.0, 1.0, B, device=dev)
    forms, keep = {}, []

    def fwd_greedy(dec):
        def step():
            with torch.no_grad():
                return dec(feats, caps)[0]
        return step

    def fwd_sample(dec, tau):
        def step():
            with torch.no_grad():
                return dec.sample(feats, T - 1, temperature=tau)[0]
        return step

    def step_greedy(dec):
        def step():
            for p in dec.parameters():
                p.grad = None
            preds, alphas = dec(feats, caps)
            loss, _ = sat_amd.caption_loss(preds, alphas, caps, 1.0, pad, skip)
            loss.backward()
            return loss
        return step

    def step_sample(dec):
        def step():
            for p in dec.parameters():
                p.grad = None
            preds, alphas, sampled = dec.sample(feats, T - 1, temperature=1.0)
            w = sat_amd.scst_weights(sampled, adv, (1,))
            loss, _ = sat_amd.weighted_caption_loss(preds, alphas, sampled, w, 0.0)
            loss.backward()
            return loss
        return step

    with torch.no_grad():
        logits, alphas0 = decoder(dev)(feats, caps)
    targets = caps[:, 1:].to(torch.int32).contiguous()
    w_fixed = torch.full((B, T - 1), 1.0 / (B * (T - 2)), device=dev)
    w_fixed[:, -1] = 0

    def loss_caption():
        x, a = logits.detach().requires_grad_(True), alphas0.detach().requires_grad_(True)
        loss, _ = sat_amd.caption_loss(x, a, caps, 1.0, pad, skip)
        loss.backward()
        return loss

    def loss_weighted():
        x, a = logits.detach().requires_grad_(True), alphas0.detach().requires_grad_(True)
        loss, _ = sat_amd.weighted_caption_loss(x, a, targets, w_fixed, 1.0)
        loss.backward()
        return loss

    for name, make in (("greedy_fwd", fwd_greedy), ("sample_fwd", lambda d: fwd_sample(d, 1.0)),
                       ("sample_fwd_t0", lambda d: fwd_sample(d, 0.0)), ("greedy_step", step_greedy),
                       ("sample_step", step_sample)):
        dec = decoder(dev)
        keep.append(dec)
        forms[name] = capture(make(dec))
    forms["loss_caption"] = capture(loss_caption)
    forms["loss_weighted"] = capture(loss_weighted)
    return forms, keep, (feats, caps)


def time_replays(graph, n):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(n):
        graph.replay()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / n


def eager_scst(B, dev, kind, steps, feats, caps):
    """The whole eager step from cached features; returns (ms per step, ms of it in the host reward)."""
    dec = decoder(dev)
    opt = sat_amd.Adam(dec.parameters(), lr=1e-5)
    refs = [[c] for c in caps.tolist()]
    cider = sat_amd.CiderD(refs, **cider_mod.PLAIN_IDS)
    ids = (0, 1, 3)

    def reward(seqs):
        if kind == "cider":
            return cider.score(seqs, range(B))
        strip = lambda c: [str(t) for t in cider_mod.strip_ids(c, *ids)]  # noqa: E731
        return [float(bleu_mod.corpus_bleu([[strip(r) for r in cider.refs[i]]], [strip(c)])) if strip(c) else 0.0
                for i, c in enumerate(seqs)]

    total = host = 0.0
    for i in range(steps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        dec.train()
        preds, alphas, sampled = dec.sample(feats, T - 1, temperature=1.0)
        dec.eval()
        with torch.no_grad():
            greedy = dec.sample(feats, T - 1, temperature=0.0)[2]
        dec.train()
        both = torch.cat([sampled, greedy]).cpu().tolist()
        h0 = time.perf_counter()
        rs, rg = reward(both[:B]), reward(both[B:])
        h1 = time.perf_counter()
        adv = torch.tensor([a - b for a, b in zip(rs, rg)], dtype=torch.float32, device=dev)
        w = sat_amd.scst_weights(sampled, adv, (1,))
        loss, _ = sat_amd.weighted_caption_loss(preds, alphas, sampled, w, 0.0)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if i >= 3:   # the first steps build lazy state
            total += time.perf_counter() - t0
            host += h1 - h0
    return 1e3 * total / steps, 1e3 * host / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scst", "step_times.json"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    dev = torch.device("cuda")
    forms, keep, (feats, caps) = build(a.batch, dev)
    for g, _ in forms.values():
        time_replays(g, 20)   # warm
    ms = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, (g, _) in forms.items():
            ms[k].append(time_replays(g, a.replays))
    out = {"shape": dict(B=a.batch, L=L, D=D, E=512, V=V, T=T, dtype="bf16", ado=True, attention=True),
           "repeats": a.repeats, "replays": a.replays, "unit": "ms per replay", "forms": {}}
    for k, v in ms.items():
        out["forms"][k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                           "runs": [round(x, 4) for x in v]}
    f = out["forms"]
    out["ratios"] = {"sample_fwd / greedy_fwd": round(f["sample_fwd"]["median"] / f["greedy_fwd"]["median"], 4),
                     "sample_fwd_t0 / greedy_fwd": round(f["sample_fwd_t0"]["median"] / f["greedy_fwd"]["median"], 4),
                     "sample_step / greedy_step": round(f["sample_step"]["median"] / f["greedy_step"]["median"], 4),
                     "loss_weighted / loss_caption": round(f["loss_weighted"]["median"] / f["loss_caption"]["median"], 4)}
    out["eager_scst_step"] = {}
    for kind in ("cider", "bleu"):
        step_ms, host_ms = eager_scst(a.batch, dev, kind, a.steps, feats, caps)
        out["eager_scst_step"][kind] = {"ms_per_step": round(step_ms, 3), "host_reward_ms": round(host_ms, 3),
                                        "host_reward_share": round(host_ms / step_ms, 4), "steps": a.steps}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

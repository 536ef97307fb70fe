"""What self-critical sequence training costs on the device, bf16, training mode, at the cfg4 shape -- B 128, L 49,
D 2048, E 512, V 10000, T 27, ado + attention -- forms replayed in turn in one process:

    greedy_fwd      the greedy forward alone (tf=False, the fused greedy step): the yardstick of the sample forward
    sample_fwd      Decoder.sample at temperature 1 alone
    sample_fwd_t0   Decoder.sample at temperature 0 (the greedy tokens through the sample instances)
    greedy_step     greedy forward + caption_loss + backward (the existing step; it must not move)
    sample_step     sample forward + weighted_caption_loss (device-resident weights) + backward
    loss_caption    caption_loss forward + backward on fixed logits
    loss_weighted   weighted_caption_loss forward + backward on the same logits
    reward_device   CiderDDevice.score of 2 B rows (a sampled and a greedy token matrix of one step), one launch
    scst_step_graph the whole SCST step as one graph: sample forward + greedy forward + reward_device + scst_weights +
                    weighted_caption_loss + backward

and the whole eager SCST step from cached features (two forwards, the reward, the loss, the backward, Adam) with the
host reward's share, for CIDEr-D and sentence BLEU-4 scored on the host and for CIDEr-D scored on the device
(cider-device: no device-to-host copy in the step) on synthetic references; the eager forms alternate, --steps steps
each per repeat.  reward_host is sat_amd.CiderD on the host over the rows reward_device scores (the copy to the host
timed apart).

    python tools/scst_bench.py [--batch 128] [--repeats 9] [--replays 100] [--steps 20] [--out FILE]

Each repeat times --replays replays of every captured form between device events, the forms alternating; the result is
the median ms per replay over the repeats with min..max.  Writes profiles/scst/step_times.json (or --out; the run
with the device reward is kept in profiles/scst_device/step_times.json) and prints it as one JSON line.
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

    # the device reward: the references are the synthetic captions, one image per row
    cider = sat_amd.CiderD([[c] for c in caps.tolist()], **cider_mod.PLAIN_IDS)
    dcider = sat_amd.CiderDDevice(cider, dev)
    images2 = torch.arange(B, device=dev, dtype=torch.int64).repeat(2)

    def step_scst(dec):
        def step():
            for p in dec.parameters():
                p.grad = None
            dec.train()
            preds, alphas, sampled = dec.sample(feats, T - 1, temperature=1.0)
            dec.eval()
            with torch.no_grad():
                greedy = dec.sample(feats, T - 1, temperature=0.0)[2]
            dec.train()
            both = torch.cat([sampled, greedy])
            r = dcider.score(both, images2)
            w = sat_amd.scst_weights(sampled, r[:B] - r[B:], (1,))
            loss, _ = sat_amd.weighted_caption_loss(preds, alphas, sampled, w, 0.0)
            loss.backward()
            return both
        return step

    dec = decoder(dev)
    keep.append(dec)
    forms["scst_step_graph"] = capture(step_scst(dec))
    forms["scst_step_graph"][0].replay()          # the captured output holds values after a replay only
    torch.cuda.synchronize()
    rows = forms["scst_step_graph"][1].clone()   # the 2 B rows of one step: what both rewards score
    forms["reward_device"] = capture(lambda: dcider.score(rows, images2))
    return forms, keep, (feats, caps, cider, dcider, rows)


def time_replays(graph, n):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(n):
        graph.replay()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / n


def eager_scst(B, dev, kind, feats, cider, dcider):
    """The whole eager step from cached features with the host reward ``kind`` (cider | bleu), or with the device
    reward (cider-device); returns run(steps) -> (ms per step, ms of it in the host reward)."""
    dec = decoder(dev)
    opt = sat_amd.Adam(dec.parameters(), lr=1e-5)
    ids = (0, 1, 3)
    images2 = torch.arange(B, device=dev, dtype=torch.int64).repeat(2)

    def reward(seqs):
        if kind == "cider":
            return cider.score(seqs, range(B))
        strip = lambda c: [str(t) for t in cider_mod.strip_ids(c, *ids)]  # noqa: E731
        return [float(bleu_mod.corpus_bleu([[strip(r) for r in cider.refs[i]]], [strip(c)])) if strip(c) else 0.0
                for i, c in enumerate(seqs)]

    def one_step():
        """-> seconds in the host reward"""
        opt.zero_grad()
        dec.train()
        preds, alphas, sampled = dec.sample(feats, T - 1, temperature=1.0)
        dec.eval()
        with torch.no_grad():
            greedy = dec.sample(feats, T - 1, temperature=0.0)[2]
        dec.train()
        if kind == "cider-device":
            r = dcider.score(torch.cat([sampled, greedy]), images2)
            adv, spent = r[:B] - r[B:], 0.0
        else:
            both = torch.cat([sampled, greedy]).cpu().tolist()
            h0 = time.perf_counter()
            rs, rg = reward(both[:B]), reward(both[B:])
            spent = time.perf_counter() - h0
            adv = torch.tensor([a - b for a, b in zip(rs, rg)], dtype=torch.float32, device=dev)
        w = sat_amd.scst_weights(sampled, adv, (1,))
        loss, _ = sat_amd.weighted_caption_loss(preds, alphas, sampled, w, 0.0)
        loss.backward()
        opt.step()
        return spent

    for _ in range(3):   # the first steps build lazy state
        one_step()

    def run(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = sum(one_step() for _ in range(steps))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, 1e3 * host / steps
    return run


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "runs": [round(x, 4) for x in v]}


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
    forms, keep, (feats, caps, cider, dcider, rows) = build(a.batch, dev)
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
    out["ratios"]["scst_step_graph / (sample_step + greedy_fwd)"] = round(
        f["scst_step_graph"]["median"] / (f["sample_step"]["median"] + f["greedy_fwd"]["median"]), 4)
    # the eager steps, alternating: --steps steps of every kind per repeat
    kinds = ("cider", "bleu", "cider-device")
    runners = {k: eager_scst(a.batch, dev, k, feats, cider, dcider) for k in kinds}
    step_ms, host_ms = {k: [] for k in kinds}, {k: [] for k in kinds}
    copy_ms, score_ms = [], []
    for _ in range(a.repeats):
        for k in kinds:
            s_ms, h_ms = runners[k](a.steps)
            step_ms[k].append(s_ms)
            host_ms[k].append(h_ms)
        torch.cuda.synchronize()   # reward_host: the copy of the 2 B rows, then CiderD on them
        t0 = time.perf_counter()
        both = rows.cpu().tolist()
        t1 = time.perf_counter()
        cider.score(both, list(range(a.batch)) * 2)
        t2 = time.perf_counter()
        copy_ms.append(1e3 * (t1 - t0))
        score_ms.append(1e3 * (t2 - t1))
    out["eager_scst_step"] = {}
    for k in kinds:
        sm, hm = statistics.median(step_ms[k]), statistics.median(host_ms[k])
        out["eager_scst_step"][k] = {"ms_per_step": round(sm, 3), "host_reward_ms": round(hm, 3),
                                     "host_reward_share": round(hm / sm, 4), "steps": a.steps,
                                     "step_ms": spread(step_ms[k]), "host_ms": spread(host_ms[k])}
    e = out["eager_scst_step"]
    out["eager_ranges_overlap"] = {"cider-device vs cider": e["cider-device"]["step_ms"]["max"]
                                   >= e["cider"]["step_ms"]["min"]}
    out["reward"] = {"rows": 2 * a.batch, "unit": "ms", "reward_host": spread(score_ms),
                     "reward_host_copy": spread(copy_ms), "reward_device": f["reward_device"],
                     "reward_host / reward_device": round(statistics.median(score_ms) / f["reward_device"]["median"], 1)}
    dev_scores = dcider.score(rows, torch.arange(a.batch, device=dev).repeat(2)).cpu().double()
    host_scores = torch.tensor(cider.score(rows.cpu().tolist(), list(range(a.batch)) * 2), dtype=torch.float64)
    out["reward"]["max_abs_err_vs_host"] = float((dev_scores - host_scores).abs().max())
    out["corpus"] = {"images": dcider.n_images, "references": dcider.n_refs, "distinct_ngrams": dcider.n_keys,
                     "table_slots": dcider.table_slots, "table_bytes": dcider.table_bytes,
                     "resident_bytes": dcider.nbytes}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What scheduled sampling costs: the decoder alone (forward + caption loss + backward as ONE captured hipGraph,
bf16, training mode) at the cfg4 shape -- B 128, L 49, D 2048, E 512, V 10000, T 27, ado + attention -- in five forms
replayed in turn in one process:

    tf_true       teacher forcing (the batched head)
    tf_false      greedy feedback (the fused greedy step): the yardstick of the sampled forms
    sampled_p0    Decoder.tf_prob = 0    (every fed token is the argmax)
    sampled_p05   Decoder.tf_prob = 0.5
    sampled_p1    Decoder.tf_prob = 1    (every fed token is the caption's)

    python tools/sched_sampling_bench.py [--batch 128] [--repeats 9] [--replays 100] [--out FILE]

Each repeat times --replays replays of every form between device events, the forms alternating; the result is the median
ms per replay over the repeats with min..max.  Writes profiles/sched_sampling/step_times.json and prints it as one JSON
line.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import sat_amd  # noqa: E402
from sat_amd.data import synthetic_captions  # noqa: E402

L, D, V, T = 49, 2048, 10000, 27
FORMS = {"tf_true": (True, None), "tf_false": (False, None), "sampled_p0": (False, 0.0), "sampled_p05": (False, 0.5),
         "sampled_p1": (False, 1.0)}


def build(B, tf, tf_prob, dev):
    torch.manual_seed(0)
    dec = sat_amd.Decoder(V, D, tf=tf, ado=True, attention=True).to(dev).train()
    dec.record_tokens = False   # as train.py: no fed-token copy per step
    dec.tf_prob = tf_prob
    feats = torch.randn(B, L, D, device=dev).relu().bfloat16()
    caps = synthetic_captions(B, T, V, generator=torch.Generator().manual_seed(1), device=dev)
    pad, skip = sat_amd.special_ids(False)

    def step():
        preds, alphas = dec(feats, caps)
        loss, _ = sat_amd.caption_loss(preds, alphas, caps, 1.0, pad, skip)
        loss.backward()
        return loss

    step()                       # lazy state (flat parameters, bf16 shadow, dropout seed) before the capture
    torch.cuda.synchronize()
    for p in dec.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    torch.cuda.synchronize()
    return graph, (dec, feats, caps, loss)


def time_replays(graph, n):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(n):
        graph.replay()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sched_sampling", "step_times.json"))
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("--repeats must be at least 7")
    dev = torch.device("cuda")
    forms = {k: build(a.batch, tf, p, dev) for k, (tf, p) in FORMS.items()}
    for g, _ in forms.values():
        time_replays(g, 20)   # warm
    ms = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, (g, _) in forms.items():
            ms[k].append(time_replays(g, a.replays))
    out = {"shape": dict(B=a.batch, L=L, D=D, E=512, V=V, T=T, dtype="bf16", ado=True, attention=True),
           "repeats": a.repeats, "replays": a.replays, "unit": "ms per forward + loss + backward replay", "forms": {}}
    for k, v in ms.items():
        loss = forms[k][1][3]
        out["forms"][k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                           "runs": [round(x, 4) for x in v], "loss_finite": bool(torch.isfinite(loss).all())}
    base = out["forms"]["tf_false"]
    for k in ("sampled_p0", "sampled_p05", "sampled_p1"):
        f = out["forms"][k]
        f["minus_tf_false_median"] = round(f["median"] - base["median"], 4)
        f["within_tf_false_min_max"] = bool(base["min"] <= f["median"] <= base["max"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

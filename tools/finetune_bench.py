"""What fine-tuning the top of the encoder costs: ONE captured hipGraph of the trainable tail's forward + the decoder
forward + caption loss + backward (+ the tail's backward), bf16, replayed in turn for every number of trainable units:
ResNet152 n = 0, 1, 2 (layer4's identity bottlenecks) and VGG19 n = 0, 4 (the block-5 convolutions).  The tail is fed
a fixed NHWC activation at plan step ``tail_start()``: the frozen prefix is not part of the step.  With n = 0 the
step is the decoder alone on fixed features (nothing of the trunk runs in it).

    python tools/finetune_bench.py [--networks resnet152,vgg19] [--batch 128] [--repeats 5] [--replays 50]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/finetune_bench.py --repeats 1 --replays 10
        (per-kernel times: conv3x3_wgrad_kernel against its floor below; no counters in that run)

Prints one JSON line: per network and n the median ms per replay and the spread (max - min) over the repeats, the
difference to n = 0, and the floors at this batch: the 3x3 weight gradient's FLOPs at 2.5 PFLOP/s (bf16 dense) and a
bottleneck's backward at twice its forward FLOPs.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import sat_amd  # noqa: E402
from sat_amd.data import synthetic_captions  # noqa: E402

PEAK_BF16_PFLOPS = 2.5
FORMS = {"resnet152": (0, 1, 2), "vgg19": (0, 4)}
TAIL_INPUT = {"resnet152": (7, 7, 2048), "vgg19": (14, 14, 512)}


def build(network, n, B, dev):
    torch.manual_seed(0)
    H, W, C = TAIL_INPUT[network]
    enc = sat_amd.Encoder(network, dtype=torch.bfloat16, fine_tune=n).to(dev).eval()
    dec = sat_amd.Decoder(10000, enc.dim, tf=True, ado=True, attention=True).to(dev).train()
    act = torch.randn(B, H, W, C, device=dev).relu().bfloat16()
    caps = synthetic_captions(B, 27, 10000, generator=torch.Generator().manual_seed(1), device=dev)
    pad, skip = sat_amd.special_ids(False)
    k, end = enc.tail_start(), enc._plan_len()
    feats0 = act.view(B, H * W, C)

    def step():
        feats = enc(act, steps=(k, end)) if n else feats0
        preds, alphas = dec(feats, caps)
        loss, _ = sat_amd.caption_loss(preds, alphas, caps, 1.0, pad, skip)
        loss.backward()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                   # lazy state (folded tail, flat parameters, bf16 shadow) before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in list(dec.parameters()) + list(enc.parameters()):
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    if n:
        assert bool(torch.isfinite(enc.tail_grad_flat).all())
    return graph, (enc, dec, act, caps)


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
    ap.add_argument("--networks", default="resnet152,vgg19")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"batch": a.batch, "repeats": a.repeats, "replays": a.replays, "networks": {}}
    for network in a.networks.split(","):
        forms = {n: build(network, n, a.batch, dev) for n in FORMS[network]}
        for g, _ in forms.values():
            time_replays(g, 5)   # warm
        ms = {n: [] for n in forms}
        for _ in range(a.repeats):   # the forms alternate
            for n, (g, _) in forms.items():
                ms[n].append(time_replays(g, a.replays))
        med = {n: statistics.median(v) for n, v in ms.items()}
        H, W, C = TAIL_INPUT[network]
        P = a.batch * H * W
        wgrad_gflop = 2.0 * P * 512 * 9 * 512 / 1e9
        rec = {"wgrad_gflop": round(wgrad_gflop, 2),
               "wgrad_floor_us": round(wgrad_gflop / PEAK_BF16_PFLOPS, 2), "n": {}}   # GFLOP / (PFLOP/s) = us
        if network == "resnet152":
            fwd = 2.0 * P * (2048 * 512 * 2 + 9 * 512 * 512) / 1e9
            rec["bottleneck_forward_gflop"] = round(fwd, 2)
            rec["bottleneck_backward_floor_us"] = round(2 * fwd / PEAK_BF16_PFLOPS, 2)
        for n in forms:
            rec["n"][str(n)] = {"ms": round(med[n], 4), "spread": round(max(ms[n]) - min(ms[n]), 4),
                                "ms_over_n0": round(med[n] - med[0], 4), "runs": [round(v, 4) for v in ms[n]]}
        out["networks"][network] = rec
        del forms
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""What the gradient with respect to the image features costs: the decoder alone (forward + caption loss +
backward as ONE captured hipGraph, bf16) with features that do and do not require grad, the two forms replayed in
turn in one process.

Instances: the benchmarked one (B 128, L 49, D 2048, E 512, V 10000, T 27, tf + ado + attention) and the cfg5
shape (L 196, D 512, E 768, V 30522, T 32, BERT, simple head).

    python tools/feature_grad_bench.py [--instances bench,cfg5] [--batch 128] [--repeats 5] [--replays 200]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/feature_grad_bench.py --repeats 1 --replays 20
        (per-kernel times: feature_grad_kernel, and the two added products among the GEMM kernels)

Prints one JSON line: per instance the median ms per replay of both forms, their spread over the repeats (max -
min), the difference, and the accumulation kernel's byte count with the time that traffic takes at 6.3 TB/s.
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

HBM_ACHIEVABLE_GBS = 6300.0
INSTANCES = {
    # name: (L, D, V, T, ado, bert)
    "bench": (49, 2048, 10000, 27, True, False),
    "cfg5": (196, 512, 30522, 32, False, True),
}


def build(name, B, requires_grad, dev):
    L, D, V, T, ado, bert = INSTANCES[name]
    torch.manual_seed(0)
    dec = sat_amd.Decoder(V, D, tf=True, ado=ado, bert=bert, attention=True).to(dev).train()
    feats = torch.randn(B, L, D, device=dev).relu().bfloat16().requires_grad_(requires_grad)
    caps = synthetic_captions(B, T, V, generator=torch.Generator().manual_seed(1), bert=bert, device=dev)
    pad, skip = sat_amd.special_ids(bert)

    def step():
        preds, alphas = dec(feats, caps)
        loss, _ = sat_amd.caption_loss(preds, alphas, caps, 1.0, pad, skip)
        loss.backward()

    step()                       # lazy state (flat parameters, bf16 shadow, dropout seed) before the capture
    torch.cuda.synchronize()
    feats.grad = None
    for p in dec.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    if requires_grad:
        assert feats.grad is not None and bool(torch.isfinite(feats.grad.float()).all())
    return graph, (dec, feats, caps)


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
    ap.add_argument("--instances", default="bench,cfg5")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"batch": a.batch, "repeats": a.repeats, "replays": a.replays, "instances": {}}
    for name in a.instances.split(","):
        L, D, V, T, ado, bert = INSTANCES[name]
        forms = {"without": build(name, a.batch, False, dev), "with": build(name, a.batch, True, dev)}
        for g, _ in forms.values():
            time_replays(g, 10)   # warm
        ms = {k: [] for k in forms}
        for _ in range(a.repeats):
            for k, (g, _) in forms.items():
                ms[k].append(time_replays(g, a.replays))
        med = {k: statistics.median(v) for k, v in ms.items()}
        B, T1 = a.batch, T - 1
        # the accumulation kernel: dctx [B (T-1), D] fp32 + alphas [B, T-1, L] fp32 + the fp32 attention.W product
        # [B L, D] read, [B, L, D] bf16 written (the [B, D] mean term is noise)
        nbytes = 4 * B * T1 * D + 4 * B * T1 * L + 4 * B * L * D + 2 * B * L * D
        out["instances"][name] = {
            "L": L, "D": D, "V": V, "T": T,
            "ms_without": round(med["without"], 4), "ms_with": round(med["with"], 4),
            "spread_without": round(max(ms["without"]) - min(ms["without"]), 4),
            "spread_with": round(max(ms["with"]) - min(ms["with"]), 4),
            "ms_difference": round(med["with"] - med["without"], 4),
            "runs_without": [round(v, 4) for v in ms["without"]], "runs_with": [round(v, 4) for v in ms["with"]],
            "accumulate_bytes": nbytes, "accumulate_floor_us": round(nbytes / (HBM_ACHIEVABLE_GBS * 1e3), 2),
            "gw_product_gflop": round(2.0 * B * L * D * dec_E(bert) / 1e9, 2),
        }
        del forms
        torch.cuda.empty_cache()
    print(json.dumps(out))


def dec_E(bert):
    return 768 if bert else 512


if __name__ == "__main__":
    main()

"""What gradient clipping by global norm costs at the benchmarked decoder shape (B=128, T=27, V=10000, ResNet152
features L=49 x D=2048, bf16), three ways, alternated in one process:
  (a) plain            sat_amd.Adam
  (b) torch_clip       torch.nn.utils.clip_grad_norm_ + sat_amd.Adam   (what a user wrote before max_grad_norm)
  (c) fused            sat_amd.Adam(max_grad_norm=C)
Every step is the eager decoder train step (forward, loss, backward, optimiser).  Device events bracket the whole step
and its optimiser part; a round runs --steps steps of each variant in turn, --rounds rounds give the spread.
    python tools/grad_clip_bench.py --out profiles/grad_clip/bench.json"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-norm", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import sat_amd
    from sat_amd.data import synthetic_captions
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench: needs an MI355X (no timing without the device)")
    dev = "cuda"
    torch.manual_seed(0)
    B, L, D, V, T = 128, 49, 2048, 10000, 27
    dec = sat_amd.Decoder(V, D, tf=True, ado=True, attention=True).to(dev).train()
    params = list(dec.parameters())
    g = torch.Generator().manual_seed(1)
    feats = (torch.randn(B, L, D, generator=g).relu()).bfloat16().to(dev)
    caps = synthetic_captions(B, T, V, generator=g, device=dev)
    pad_id, skip_ids = sat_amd.special_ids(False)
    opts = {"plain": sat_amd.Adam(params, lr=1e-4), "torch_clip": sat_amd.Adam(params, lr=1e-4),
            "fused": sat_amd.Adam(params, lr=1e-4, max_grad_norm=args.max_norm)}

    def step(name, events=None):
        opt = opts[name]
        if events:
            events[0].record()
        opt.zero_grad()
        preds, alphas = dec(feats, caps)
        loss, _ = sat_amd.caption_loss(preds, alphas, caps, pad_id=pad_id, skip_ids=skip_ids)
        loss.backward()
        if events:
            events[1].record()
        if name == "torch_clip":
            torch.nn.utils.clip_grad_norm_(params, args.max_norm)
        opt.step()
        if events:
            events[2].record()

    for _ in range(args.warmup):
        for name in opts:
            step(name)
    torch.cuda.synchronize()
    n_grad = sum(p.grad.numel() for p in params if p.grad is not None)
    rounds = {name: {"step_us": [], "opt_us": []} for name in opts}
    for _ in range(args.rounds):
        for name in opts:
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
            for e in evs:
                step(name, e)
            torch.cuda.synchronize()
            rounds[name]["step_us"].append(1e3 * sum(e[0].elapsed_time(e[2]) for e in evs) / args.steps)
            rounds[name]["opt_us"].append(1e3 * sum(e[1].elapsed_time(e[2]) for e in evs) / args.steps)

    def stats(xs):
        return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}

    def diff(a, b, key):
        return stats([x - y for x, y in zip(rounds[a][key], rounds[b][key])])

    out = {"shape": dict(B=B, L=L, D=D, V=V, T=T, dtype="bf16"), "gradient_elements": n_grad,
           "steps_per_round": args.steps, "rounds": args.rounds, "max_norm": args.max_norm, "unit": "us per step",
           "grad_norm": float(opts["fused"].grad_norm), "clip_scale": float(opts["fused"].clip_scale),
           "variants": {name: {k: stats(v) for k, v in r.items()} for name, r in rounds.items()},
           "fused_minus_plain": {k: diff("fused", "plain", k) for k in ("step_us", "opt_us")},
           "torch_clip_minus_fused": {k: diff("torch_clip", "fused", k) for k in ("step_us", "opt_us")},
           "per_round": rounds}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

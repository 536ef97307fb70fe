"""Caption throughput: a loop of single-image beam searches against one batched beam search.

    python tools/caption_bench.py                       # COCO shape, N = 64, beam 3, bf16 and fp32
    python tools/caption_bench.py --bert --beam 5 --only batch --dtypes bf16   # for a kernel trace

Both sides decode the same N images (random weights, random features) in one process:
  (a) ``Decoder.caption`` once per image, on the image's features expanded to beam rows
  (b) ``Decoder.caption_batch`` once for all N images
Random weights almost never complete a beam, so both sides run all max_step + 1 steps; the steps each
side ran are printed (a search that returns score -inf ran them all, one that completed ran at least
its sentence length - 1).  Each side is warmed up once, then timed ``--repeats`` times, alternating
the sides, with a device synchronise before and after each timed call; the medians are reported.
Prints one JSON line per dtype.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import contextlib
import io
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sat_amd  # noqa: E402


def steps_run(results, max_step):
    """Decoder steps the searches behind ``results`` [(ids, score)] took: (min over images, max over images)."""
    per = [max_step + 1 if math.isinf(score) else len(ids) - 1 for ids, score in results]
    return min(per), max(per)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--images", type=int, default=64)
    p.add_argument("--beam", type=int, default=3)
    p.add_argument("--max-step", type=int, default=50)
    p.add_argument("--L", type=int, default=49)
    p.add_argument("--D", type=int, default=2048)
    p.add_argument("--vocab", type=int, default=10000)
    p.add_argument("--bert", action="store_true", help="BERT decoder (V = 30522, E = 768)")
    p.add_argument("--no-ado", action="store_true")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--dtypes", nargs="+", choices=["bf16", "fp32"], default=["bf16", "fp32"])
    p.add_argument("--only", choices=["both", "batch"], default="both", help="batch: skip the single-image loop")
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("caption_bench: no GPU")
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    N, R, L, D = args.images, args.beam, args.L, args.D
    dec = sat_amd.Decoder(args.vocab, D, ado=not args.no_ado, bert=args.bert, attention=True).to(dev).eval()
    feats32 = torch.randn(N, L, D, device=dev)
    for name in args.dtypes:
        feats = feats32.bfloat16() if name == "bf16" else feats32
        expanded = [feats[i:i + 1].expand(R, L, D).contiguous() for i in range(N)]

        def single():
            out = []
            for f in expanded:
                ids, _ = dec.caption(f, R, args.max_step)
                out.append((ids, dec.last_caption_score))
            return out

        def batch():
            return [(ids, score) for ids, _, score in dec.caption_batch(feats, R, args.max_step, max_images=N)]

        sides = {"batch": batch} if args.only == "batch" else {"single": single, "batch": batch}
        times = {k: [] for k in sides}
        steps = {}
        with contextlib.redirect_stdout(io.StringIO()):   # the "no completed sentence" notices
            for k, fn in sides.items():   # warm-up: code objects, workspaces, the bf16 weight shadow
                _, out = timed(fn)
                steps[k] = steps_run(out, args.max_step)
            for _ in range(args.repeats):
                for k, fn in sides.items():
                    times[k].append(timed(fn)[0])
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"dtype": name, "images": N, "beam": R, "max_step": args.max_step, "L": L, "D": D,
               "V": dec.vocabulary_size, "E": dec.embedding_size, "repeats": args.repeats,
               "batch_seconds": med["batch"], "batch_seconds_all": times["batch"],
               "batch_captions_per_s": N / med["batch"], "batch_steps_min_max": steps["batch"],
               "batch_us_per_step": med["batch"] / steps["batch"][1] * 1e6}
        if "single" in sides:
            rec.update({"single_seconds": med["single"], "single_seconds_all": times["single"],
                        "single_captions_per_s": N / med["single"], "single_steps_min_max": steps["single"],
                        "ratio": med["single"] / med["batch"]})
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

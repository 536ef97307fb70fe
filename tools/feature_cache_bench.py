"""Measurements behind DESIGN 4.15 (the feature cache), on one MI355X.

    python tools/feature_cache_bench.py [--out profiles/feature_cache] [--parts a,b,c]

  a  sat_rows_gather at the benchmarked shape: n = 128 rows of 100,352 bf16 elements, random slots of a 4096-row table
     (822 MB: larger than the 256 MiB Infinity Cache), 50 back-to-back calls per timing, 7 timings; the same for
     torch.index_select on the same data.  us per call and the fraction of the 6.29 TB/s copy rate, counting the
     bytes read plus the bytes written.                                                        -> rows_gather.json
  b  train.py's own step loop (train_epoch), ResNet152, bf16, B = 128, V = 10000, T = 27, 100 steps: the uncached
     form (encoded_batches, overlap on: images from pinned host batches, the trunk one batch ahead on the side
     stream) against the cached form (cached_batches over a 4096-image FeatureCache).  The two alternate three times
     in this one process; ms per step of every run, the medians and the spread (max - min).    -> train_step.json
  c  torch.cuda.max_memory_allocated() of the default (uncached) step at B = 128 for both networks: the figure
     FeatureCache.RESERVE_BYTES is sized from.                                                 -> step_memory.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import sat_amd  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s, the measured float4 copy rate of the chip
ROW, N, TABLE_ROWS = 100_352, 128, 4096


def train_module():
    spec = importlib.util.spec_from_file_location("sat_train_cli_bench",
                                                  os.path.join(REPO, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def part_a(dev):
    g = torch.Generator().manual_seed(0)
    table = torch.empty(TABLE_ROWS, ROW, dtype=torch.bfloat16, device=dev)
    table.view(torch.int16).random_(0, 16000)   # finite bf16 bit patterns; the values do not matter
    idxs = [torch.randint(0, TABLE_ROWS, (N,), generator=g).to(dev) for _ in range(50)]
    out = torch.empty(N, ROW, dtype=torch.bfloat16, device=dev)
    moved = 2 * N * ROW * 2   # bytes read + bytes written per call

    def ours(i):
        sat_amd.ops.rows_gather(table, i, out=out)

    def torchs(i):
        torch.index_select(table, 0, i, out=out)

    res = {"n": N, "row_elems": ROW, "table_rows": TABLE_ROWS, "dtype": "bf16", "bytes_per_call": moved,
           "floor_us": moved / COPY_RATE * 1e6}
    for name, fn in (("rows_gather", ours), ("index_select", torchs)):
        fn(idxs[0])
        assert torch.equal(out.view(torch.int16), table[idxs[0]].view(torch.int16))
        times = []
        for _ in range(7):
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            st.record()
            for i in idxs:
                fn(i)
            en.record()
            torch.cuda.synchronize()
            times.append(st.elapsed_time(en) * 1e3 / len(idxs))
        us = statistics.median(times)
        res[name] = {"us_per_call": us, "us_min": min(times), "us_max": max(times),
                     "fraction_of_copy_rate": moved / (us * 1e-6) / COPY_RATE}
    return res


def setup(T, network, dev):
    args = T.parse(["--synthetic", "512", "--network", network, "--tf", "--ado", "--attention", "--batch-size", str(N),
                    "--vocab", "10000", "--seq", "27", "--log-interval", "1000000"])
    T.set_seed(args.seed)
    encoder, decoder, _, dt = T.build(args, dev)
    decoder.record_tokens = False
    decoder.split_target = 128 if network == "vgg19" else 96   # train.py main(), overlap on, B > 64
    encoder.fuse_blocks = False
    opt = sat_amd.Adam(decoder.parameters(), lr=args.lr)
    g = torch.Generator().manual_seed(1)
    images = [torch.randn(N, 3, 224, 224, generator=g).pin_memory() for _ in range(4)]
    caps = [sat_amd.data.synthetic_captions(N, 27, 10000, generator=g).pin_memory() for _ in range(4)]
    return args, encoder, decoder, opt, dt, images, caps


def run_epoch(T, args, encoder, decoder, opt, dt, dev, loader, cache=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.train_epoch(1, encoder, decoder, opt, loader, args, dev, dt, 1, lambda rec: None, None, cache)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(loader)


def part_b(T, dev, steps=100):
    args, encoder, decoder, opt, dt, images, caps = setup(T, "resnet152", dev)
    uncached = [(images[i % 4], caps[i % 4], None) for i in range(steps)]
    cache = sat_amd.FeatureCache(encoder, range(TABLE_ROWS), dt, N)
    t0 = time.perf_counter()
    cache.fill([images[i % 4] for i in range(TABLE_ROWS // N)])
    torch.cuda.synchronize()
    fill_s = time.perf_counter() - t0
    g = torch.Generator().manual_seed(2)
    cached = [(torch.randint(0, TABLE_ROWS, (N,), generator=g), caps[i % 4], None) for i in range(steps)]
    for loader, c in ((uncached[:20], None), (cached[:20], cache)):   # warm-up: plans, workspaces, allocator
        run_epoch(T, args, encoder, decoder, opt, dt, dev, loader, c)
    runs = {"uncached": [], "cached": []}
    for _ in range(3):
        runs["uncached"].append(run_epoch(T, args, encoder, decoder, opt, dt, dev, uncached))
        runs["cached"].append(run_epoch(T, args, encoder, decoder, opt, dt, dev, cached, cache))
    res = {"network": "resnet152", "dtype": "bf16", "batch": N, "vocab": 10000, "seq": 27, "steps": steps,
           "cache_images": TABLE_ROWS, "cache_bytes": cache.nbytes, "fill_seconds": fill_s,
           "fill_images_per_second": TABLE_ROWS / fill_s}
    for name, ms in runs.items():
        res[name] = {"ms_per_step": ms, "median": statistics.median(ms), "spread": max(ms) - min(ms)}
    res["speedup_of_medians"] = res["uncached"]["median"] / res["cached"]["median"]
    return res


def part_c(T, dev, steps=12):
    res = {"batch": N, "dtype": "bf16", "vocab": 10000, "seq": 27}
    for network in ("resnet152", "vgg19"):
        args, encoder, decoder, opt, dt, images, caps = setup(T, network, dev)
        loader = [(images[i % 4], caps[i % 4], None) for i in range(steps)]
        run_epoch(T, args, encoder, decoder, opt, dt, dev, loader)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        run_epoch(T, args, encoder, decoder, opt, dt, dev, loader)
        res[network] = {"max_memory_allocated": torch.cuda.max_memory_allocated(dev),
                        "allocated_between_steps": base}
        del encoder, decoder, opt, loader
        torch.cuda.empty_cache()
    res["reserve_bytes"] = sat_amd.feature_cache.RESERVE_BYTES
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "feature_cache"))
    ap.add_argument("--parts", default="a,b,c")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda", 0)
    parts = a.parts.split(",")
    T = train_module()
    for part, name, fn in (("a", "rows_gather", lambda: part_a(dev)), ("b", "train_step", lambda: part_b(T, dev)),
                           ("c", "step_memory", lambda: part_c(T, dev))):
        if part in parts:
            res = fn()
            with open(os.path.join(a.out, name + ".json"), "w") as f:
                json.dump(res, f, indent=1)
            print(json.dumps({name: res}), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

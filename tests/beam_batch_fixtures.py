"""Shared fixtures of the batched beam-search tests (test_cpu_beam_batch_fixtures.py proves them
fit for an ids comparison, test_gpu_beam_batch.py runs them on the device).

A set = the weights of one beam golden (golden_util.load_beam) + several images: the golden's own
features first, then features drawn from the committed seeds below exactly as make_golden_beam.py
draws its one image (``default_rng(seed).standard_normal((1, L, D))``).  The expected value of an
image is ``oracle.beam_search`` on its features expanded to beam rows, in fp32.

The seeds were picked with the oracle alone so that set A mixes short, long and never-completing
sentences and every image's fp32 and fp64 searches agree (no top-k margin inside rounding noise):
  set A at max_step=50: lengths 30, 4, 11, 8, 17, none, 41; at max_step=6 the golden image, 1008 and
  1001 do not complete, 1007 / 1013 / 1022 do, and 1017 completes at the last step allowed (7).
"""
import functools
import os

import numpy as np
import torch

import golden_util as G

SETS = {
    "A": ("att_simple_b3", (1007, 1013, 1017, 1008, 1001, 1022)),
    "B_ado": ("att_ado_b5", (1002, 1000, 1013)),
    "B_noatt": ("noatt_simple_b4", (1006, 1001)),
    "B_bert": ("bert_att_ado_b3", (1001, 1013, 1000, 1014)),
    "beam1": ("att_simple_b1", ()),
}
MAX_STEPS = (50, 6)


@functools.lru_cache(maxsize=None)
def load(set_name):
    """(golden dict with cfg / params, features [N, L, D] fp32: the golden image first)."""
    golden, seeds = SETS[set_name]
    g = G.load_beam(os.path.join(G.GOLDEN, f"beam_{golden}.npz"))
    cfg = g["cfg"]
    imgs = [torch.from_numpy(g["img_features"])]
    for seed in seeds:
        imgs.append(torch.from_numpy(np.random.default_rng(seed).standard_normal(
            (1, cfg["L"], cfg["D"])).astype(np.float32)))
    return g, torch.cat(imgs, 0).contiguous()


@functools.lru_cache(maxsize=None)
def expected(set_name, max_step, double=False):
    """Per image (ids, alpha rows [rows, L] float64 array, score) from oracle.beam_search; computed once
    per process and shared (treat as read-only).  ``double``: params and features cast to float64."""
    from oracle import sat_oracle as O
    g, feats = load(set_name)
    cfg, p = g["cfg"], g["params"]
    if double:
        p = {k: v.double() for k, v in p.items()}
        feats = feats.double()
    out = []
    with torch.no_grad():
        for i in range(feats.shape[0]):
            f = feats[i:i + 1].expand(cfg["beam"], cfg["L"], cfg["D"]).contiguous()
            ids, al, score = O.beam_search(p, f, cfg["beam"], ado=cfg["ado"], attention=cfg["attention"],
                                           bert=cfg["bert"], max_step=max_step)
            out.append((ids, np.asarray(al, dtype=np.float64), score))
    return out

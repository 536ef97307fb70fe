"""Image batches and output sizes that reach every path of sat_images_to_input (csrc/images.hip), and a restatement
of what its launch does with them: the batch's tap counts, the LDS bytes it asks for, and how a 16-row tile splits into
chunks of the 48-row LDS window.  tests/test_cpu_image_cases.py proves on the CPU that each case reaches the path it is
in the table for and that the oracle (oracle/pil_resize.py) equals PIL on every image; tests/test_gpu_image_input.py
compares the kernel with the oracle bit for bit.  No GPU use here.

Every image has h <= 100 w: above that Pillow 12's Image.resize runs the vertical pass first (oracle/pil_resize.py),
and the kernel and the oracle are horizontal first.  No image has more than 1.2 M pixels: the oracle's einsum
materialises [H, out, ksize, 3] in int64.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import pil_resize as PR

# csrc/images.hip
TY = 16              # output rows per workgroup
RCAP = 48            # horizontally resampled rows held in LDS
KMAX = 32            # taps per output index
MAX_OW = 512
LDS_LIMIT = 163840   # 160 KiB per workgroup on the MI355X
MAX_PIXELS = 1200000

# name, [(h, w), ...], (OH, OW), why: the path the case is in the table for; gpu: False = the launch must be refused
Case = namedtuple("Case", "name sizes out why gpu")


def _table():
    cs = [
        Case("small_taps", [(1, 1), (2, 3), (224, 224), (223, 225), (225, 223), (224, 300), (300, 224), (448, 448),
                            (672, 672), (1, 500), (500, 5)], (224, 224), "register", True),
        Case("deep", [(3360, 34), (34, 3360), (3359, 35), (3137, 40), (1000, 231), (900, 1000), (7, 9)], (224, 224),
             "deep", True),
        Case("edge_9tap", [(673, 672), (672, 673)], (224, 224), "edge9", True),
        Case("out40x24", [(111, 97), (600, 360)], (40, 24), "partial15x", True),
        Case("out33x17", [(37, 53)], (33, 17), "odd", True),
        Case("out34x50", [(480, 640)], (34, 50), "size", True),
        Case("out2x2", [(20, 30)], (2, 2), "size", True),
        Case("out16x16", [(31, 29)], (16, 16), "size", True),
        Case("out1x1", [(15, 15)], (1, 1), "size", True),
        Case("out256x256", [(640, 480)], (256, 256), "size", True),
        Case("out48x512", [(90, 1500)], (48, 512), "size", True),
        Case("out18x512_fits", [(2, 6656)], (18, 512), "lds_fits", True),
        Case("out18x512_over", [(100, 7680)], (18, 512), "lds_over", False),
        # the limit itself: 29 horizontal taps fit beside 29 vertical ones with 64 bytes to spare, not beside 31
        Case("out2x512_fits", [(28, 6657)], (2, 512), "lds_fits", True),
        Case("out2x512_over", [(30, 6657)], (2, 512), "lds_over", False),
    ]
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
GPU_CASES = [c for c in CASES if c.gpu]
REFUSED = [c for c in CASES if not c.gpu]


def images(case):
    """The case's images: uint8 [h, w, 3] from a generator seeded by the case's name."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in case.sizes]


def s2d_ok(case):
    return case.out[0] % 2 == 0 and case.out[1] % 2 == 0


# ---------------------------------------------------------------------------- what the launch does
@functools.lru_cache(maxsize=None)
def _coeffs(in_size, out_size):
    return PR.coeffs(in_size, out_size)


def ksize(in_size, out_size):
    """Taps per output index: ceil(max(in / out, 1)) * 2 + 1, the width of the oracle's table."""
    return _coeffs(in_size, out_size)[2].shape[1]


def taps(sizes, out):
    """(KH, KV) of a batch: sized from its widest and its tallest image (launch_resample)."""
    OH, OW = out
    return ksize(max(w for _, w in sizes), OW), ksize(max(h for h, _ in sizes), OH)


def lds_bytes(sizes, out):
    """LDS bytes the launch asks for: the row window, the horizontal table, the tile's vertical table."""
    KH, KV = taps(sizes, out)
    OW = out[1]
    return RCAP * OW * 4 + OW * (2 + KH) * 4 + TY * (2 + KV) * 4


def n_tiles(OH):
    return -(-OH // TY)


def chunk_plan(h, OH, tile, s2d):
    """How the workgroup of output rows [tile * TY, min(tile * TY + TY, OH)) of an image of height h walks them:
    [(first row, end row, LDS rows the chunk's input span needs)], the kernel's loop over vlo / vn.  ``s2d``: the
    S2D16 layout, whose chunks hold whole row pairs."""
    lo, n, _ = _coeffs(h, OH)
    y0 = tile * TY
    yend = min(y0 + TY, OH)
    step = 2 if s2d else 1
    plan = []
    ys = y0
    while ys < yend:
        r0 = lo[ys]
        ye = ys + step
        while ye + step <= yend and lo[ye + step - 1] + n[ye + step - 1] - r0 <= RCAP:
            ye += step
        plan.append((ys, ye, int(lo[ye - 1] + n[ye - 1] - r0)))
        ys = ye
    return plan


def plans(case, s2d):
    """Every (image, tile)'s chunk plan."""
    OH = case.out[0]
    return [chunk_plan(h, OH, t, s2d) for h, _ in case.sizes for t in range(n_tiles(OH))]

"""The image-input case table (tests/image_cases.py) checked on the CPU: every case reaches the path of
sat_images_to_input it is in the table for (asserted from a restatement of the launch: tap counts, LDS bytes, chunk
plan), the oracle equals PIL on every image of every case, and Pillow's vertical-first rule for images with
h > 100 w -- which the table keeps out -- is pinned.  No GPU.

What a chunk can span.  At the 15x limit an output row has at most 30 taps (xmax - xmin <= 2 * support = 30) and
consecutive rows start at most 15 input rows apart, so two rows -- an S2D16 row pair, or two NCHW rows -- span at most
45 input rows and three rows at least 58: a chunk of the 48-row window then holds exactly two rows, a 16-row tile
splits into 8 chunks (the most any accepted image can give), and the span of 45 is the widest a one-pair chunk gets.
The window itself is filled to exactly 48 rows by shallower images whose chunks hold several rows.
"""
import numpy as np
import pytest

import image_cases as IC
from oracle import pil_resize as PR

IDS = [c.name for c in IC.CASES]


# KH, KV and LDS bytes at 512 columns, either side of the 163,840-byte limit
LDS_FIGURES = {"out18x512_fits": (27, 3, 158016), "out18x512_over": (31, 13, 166848),
               "out2x512_fits": (29, 29, 163776), "out2x512_over": (29, 31, 163904)}


def test_table_is_the_one_the_tests_rely_on():
    assert [c.name for c in IC.REFUSED] == ["out18x512_over", "out2x512_over"]
    assert {c.name for c in IC.CASES if c.why in ("lds_fits", "lds_over")} == set(LDS_FIGURES)
    assert {c.why for c in IC.CASES} == {"register", "deep", "edge9", "partial15x", "odd", "size", "lds_fits",
                                         "lds_over"}
    assert (IC.TY, IC.RCAP, IC.KMAX, IC.MAX_OW, IC.LDS_LIMIT) == (16, 48, 32, 512, 160 * 1024)


@pytest.mark.parametrize("case", IC.CASES, ids=IDS)
def test_case_constraints(case):
    """Every image: h <= 100 w (PIL's tall-image rule stays out), at most 1.2 M pixels (the oracle's einsum), within
    the kernel's 15x downscale and 512-column limits."""
    OH, OW = case.out
    assert 0 < OW <= IC.MAX_OW and OH > 0
    for h, w in case.sizes:
        assert h <= 100 * w, (case.name, h, w)
        assert h * w <= IC.MAX_PIXELS, (case.name, h, w)
        assert h <= 15 * OH and w <= 15 * OW, (case.name, h, w)
    KH, KV = IC.taps(case.sizes, case.out)
    assert KH <= IC.KMAX and KV <= IC.KMAX


@pytest.mark.parametrize("case", IC.CASES, ids=IDS)
def test_case_reaches_its_path(case):
    KH, KV = IC.taps(case.sizes, case.out)
    lds = IC.lds_bytes(case.sizes, case.out)
    OH, OW = case.out
    nchw = IC.plans(case, False)
    s2d = IC.plans(case, True) if IC.s2d_ok(case) else []
    print(f"{case.name}: KH {KH} KV {KV} LDS {lds} B, chunks per tile <= {max(len(p) for p in nchw)}, "
          f"widest chunk {max(r for p in nchw + s2d for _, _, r in p)} rows")
    # no chunk of any accepted image outgrows the window (the kernel's nrows > RCAP guard stays unreachable), and
    # every tile's chunks cover its rows once
    for p, step in [(p, 1) for p in nchw] + [(p, 2) for p in s2d]:
        assert all(0 < r <= IC.RCAP for _, _, r in p), (case.name, p)
        assert all(a[1] == b[0] for a, b in zip(p, p[1:])) and all((ye - ys) % step == 0 for ys, ye, _ in p)
        assert p[0][0] % IC.TY == 0 and p[-1][1] == min(p[0][0] + IC.TY, OH)
    if OH % IC.TY:   # a partial last tile
        last = [p for p in nchw if p[-1][1] == OH]
        assert last and all(p[-1][1] - p[0][0] == OH % IC.TY for p in last)
    if case.gpu:
        assert lds <= IC.LDS_LIMIT, (case.name, lds)
    else:
        assert lds > IC.LDS_LIMIT, (case.name, lds)
    why = case.why
    if why == "register":
        assert KH <= 8 and KV <= 8
        assert {IC.ksize(w, OW) for _, w in case.sizes} >= {3, 5, 7}   # 1, 2 and 3 x support in one batch
    elif why == "edge9":
        assert KH == 9 and KV == 9
        assert all(IC.taps([s], case.out) in ((9, 7), (7, 9)) for s in case.sizes)   # each image is past it on one axis
    elif why == "deep":
        assert KH == 31 and KV == 31
        assert any(IC.taps([s], case.out)[0] <= 5 for s in case.sizes)   # a narrow image rides the looped path
        # one row pair per S2D16 chunk at the widest span a pair can have, 8 chunks per tile in both layouts
        assert any((ye - ys, r) == (2, 45) for p in s2d for ys, ye, r in p)
        assert any(len(p) == IC.TY // 2 and all(ye - ys == 2 for ys, ye, _ in p) for p in s2d)
        assert any(len(p) == IC.TY // 2 for p in nchw) and max(len(p) for p in nchw + s2d) == IC.TY // 2
        # ... and a chunk that fills the window to its last row
        assert any(r == IC.RCAP for p in nchw for _, _, r in p)
    elif why == "partial15x":
        assert KH == 31 and KV == 31 and OH % IC.TY == 8
        assert all(len(p) == 4 for p in nchw if p[-1][1] == OH and len(p) > 1)   # the 15x image's 8-row tile
        assert any(len(p) == 4 for p in nchw)
    elif why == "odd":
        assert not IC.s2d_ok(case) and OH % 2 == 1 and OW % 2 == 1
    elif why in ("lds_fits", "lds_over"):
        assert OW == IC.MAX_OW and (KH, KV, lds) == LDS_FIGURES[case.name]


def test_library_reports_the_same_lds_bytes():
    """sat_images_lds_bytes (the figure the entry point refuses on) is the restatement's, on either side of the limit;
    without a device the limit is the 160 KiB floor."""
    import sat_amd
    lib = sat_amd._lib.lib()
    for case in IC.CASES:
        mh, mw = max(h for h, _ in case.sizes), max(w for _, w in case.sizes)
        assert lib.sat_images_lds_bytes(mh, mw, *case.out) == IC.lds_bytes(case.sizes, case.out), case.name
    assert lib.sat_images_lds_bytes(0, 5, 4, 4) == 0 and lib.sat_images_lds_bytes(5, 5, 4, 0) == 0
    assert lib.sat_images_lds_limit() >= IC.LDS_LIMIT


def test_table_covers_every_output_shape_class():
    outs = [c.out for c in IC.GPU_CASES]
    assert any(OH % IC.TY for OH, _ in outs) and any(OH < IC.TY for OH, _ in outs) and (1, 1) in outs and (2, 2) in outs
    assert any(OW == IC.MAX_OW for _, OW in outs) and any(OH != OW for OH, OW in outs)
    assert any(OH > 224 for OH, _ in outs)
    sizes = [(s, c.out) for c in IC.GPU_CASES for s in c.sizes]
    assert any(h == 1 for (h, w), _ in sizes) and any(w == 1 for (h, w), _ in sizes)          # a 1-pixel axis
    assert any(h == 2 and OH == 224 for (h, w), (OH, OW) in sizes)                            # 2 -> 224
    assert any((h == OH) != (w == OW) for (h, w), (OH, OW) in sizes)                          # in == out on one axis
    assert any(h < OH and w > OW for (h, w), (OH, OW) in sizes)                               # up one way, down the other


# ---------------------------------------------------------------------------- the oracle against PIL
def _pil(img, size):
    Image = pytest.importorskip("PIL.Image")   # the coverage tests above need no PIL
    OH, OW = size
    return np.asarray(Image.fromarray(img, "RGB").resize((OW, OH), Image.BILINEAR))


@pytest.mark.parametrize("case", IC.CASES, ids=IDS)
def test_oracle_equals_pil_on_every_image(case):
    for img in IC.images(case):
        got = PR.resize_bilinear(img, case.out)
        assert got.dtype == np.uint8 and got.shape == case.out + (3,)
        assert np.array_equal(got, _pil(img, case.out)), (case.name, img.shape)


def _vertical_first(img, size):
    OH, OW = size
    return PR._pass(PR._pass(img, 0, OH), 1, OW)


def test_tall_image_rule_boundary():
    """h <= 100 w: PIL resamples horizontally first, as the oracle and the kernel do."""
    img = np.random.default_rng(600).integers(0, 256, (600, 9, 3), dtype=np.uint8)
    assert np.array_equal(PR.resize_bilinear(img, (224, 224)), _pil(img, (224, 224)))


@pytest.mark.parametrize("h,w", [(1000, 9), (3360, 9)])
def test_tall_image_rule(h, w):
    """h > 100 w and a shrinking height: Pillow 12's Image.resize resamples vertically first, so the horizontal-first
    oracle (and the kernel) differ from it by 1 in some bytes, and the oracle's own passes composed vertical first
    equal it exactly."""
    import PIL
    size = (224, 224)
    img = np.random.default_rng(h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = _pil(img, size)
    hfirst = PR.resize_bilinear(img, size)
    if np.array_equal(hfirst, ref):
        pytest.skip(f"Pillow {PIL.__version__} resamples {h}x{w} horizontally first: it lacks the tall-image rule")
    diff = np.abs(hfirst.astype(np.int16) - ref.astype(np.int16))
    print(f"{h}x{w}: Pillow {PIL.__version__}, {100 * (diff != 0).mean():.1f} % of the bytes differ, max {diff.max()}")
    assert diff.max() == 1
    assert np.array_equal(_vertical_first(img, size), ref)

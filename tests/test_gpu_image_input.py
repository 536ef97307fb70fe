"""sat_images_to_input (csrc/images.hip) against the CPU oracle of Pillow's resampler + ToTensor + Normalize
(oracle/pil_resize.py, itself pinned against PIL on these very images by tests/test_cpu_image_cases.py), bit for bit,
on every case of tests/image_cases.py: both tap-count paths and batches that mix them, chunks at the widest spans the
48-row LDS window sees, partial and single-row tiles, odd and 512-column outputs, both store paths of the NHWC
epilogue, S2D16, and the LDS limit from either side.  The NHWC and S2D16 expectations are built with torch alone
(permute / reshape / zero padding / .to(dtype)); sat_nchw_to_nhwc and sat_nchw_to_s2d, which the older test builds
its expectations with, are compared with the same constructions here.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_cases as IC
from oracle import pil_resize as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
GPU_IDS = [c.name for c in IC.GPU_CASES]
S2D_CASES = [c for c in IC.GPU_CASES if IC.s2d_ok(c)]
INVALID = "9001"   # SAT_ERR_INVALID: returned by the entry point's argument checks, all of them before its first launch


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


# ---------------------------------------------------------------------------- expectations, torch and numpy alone
_REF = {}


def reference(case):
    """(images, the oracle's [B, 3, OH, OW] float32 tensor), computed once per case and never written to."""
    if case.name not in _REF:
        imgs = IC.images(case)
        _REF[case.name] = (imgs, torch.from_numpy(np.stack([PR.transform(a, case.out) for a in imgs])))
    return _REF[case.name]


def nhwc_of(x, c_pad, dtype):
    """[N, C, H, W] f32 -> [N, H, W, c_pad] (dtype), channels >= C zero."""
    N, C, H, W = x.shape
    y = torch.zeros(N, H, W, c_pad, dtype=torch.float32)
    y[..., :C] = x.permute(0, 2, 3, 1)
    return y.to(dtype)


def s2d16_of(x, dtype):
    """[N, C, H, W] f32 -> [N, H/2, W/2, 16] (dtype), channel (sy * 2 + sx) * C + c, channels >= 4 C zero."""
    N, C, H, W = x.shape
    y = torch.zeros(N, H // 2, W // 2, 16, dtype=torch.float32)
    y[..., :4 * C] = x.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(N, H // 2, W // 2, 4 * C)
    return y.to(dtype)


def same_bits(got, want):
    """Equal as numbers and as bit patterns (a -0.0 in a pad channel is not a zero)."""
    got = got.cpu()
    ib = torch.int16 if want.dtype == BF else torch.int32
    return (got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
            and torch.equal(got.contiguous().view(ib), want.contiguous().view(ib)))


def _packed(sat, imgs):
    return sat.PackedImages.from_arrays(imgs).to(DEV)


# ---------------------------------------------------------------------------- every case, every layout
@pytest.mark.parametrize("case", IC.GPU_CASES, ids=GPU_IDS)
def test_nchw(sat, case):
    from sat_amd import ops, _lib as Lb
    imgs, ref = reference(case)
    got = ops.images_to_input(_packed(sat, imgs), Lb.IMG_NCHW, F32, size=case.out)
    assert same_bits(got, ref)


@pytest.mark.parametrize("case", IC.GPU_CASES, ids=GPU_IDS)
def test_nhwc_16_byte_stores(sat, case):
    """c_pad * sizeof(T) == 16: one 16-byte store per pixel."""
    from sat_amd import ops, _lib as Lb
    imgs, ref = reference(case)
    packed = _packed(sat, imgs)
    for dt, c_pad in ((BF, 8), (F32, 4)):
        got = ops.images_to_input(packed, Lb.IMG_NHWC, dt, c_pad=c_pad, size=case.out)
        assert same_bits(got, nhwc_of(ref, c_pad, dt)), (dt, c_pad)
        assert not got[..., 3:].any()


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", ["small_taps", "out40x24"])
def test_nhwc_every_pad(sat, name, dt):
    """The scalar epilogue (c_pad 3, 64 and one of 4 / 8 per dtype) beside the 16-byte one; pad channels exactly 0."""
    from sat_amd import ops, _lib as Lb
    case = IC.BY_NAME[name]
    imgs, ref = reference(case)
    packed = _packed(sat, imgs)
    for c_pad in (3, 4, 8, 64):
        got = ops.images_to_input(packed, Lb.IMG_NHWC, dt, c_pad=c_pad, size=case.out)
        assert same_bits(got, nhwc_of(ref, c_pad, dt)), c_pad
        assert not got[..., 3:].any()


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", S2D_CASES, ids=[c.name for c in S2D_CASES])
def test_s2d16(sat, case, dt):
    from sat_amd import ops, _lib as Lb
    imgs, ref = reference(case)
    got = ops.images_to_input(_packed(sat, imgs), Lb.IMG_S2D16, dt, size=case.out)
    assert same_bits(got, s2d16_of(ref, dt))
    assert not got[..., 12:].any()


@pytest.mark.parametrize("name", ["small_taps", "deep"])
def test_image_alone_equals_its_row_in_the_batch(sat, name):
    """KH / KV are sized from the batch: an image resized alone, with tap counts of its own (and, for the narrow images
    of ``deep``, on the other horizontal path), gives the bytes of its row in the mixed batch."""
    from sat_amd import ops, _lib as Lb
    case = IC.BY_NAME[name]
    imgs, ref = reference(case)
    packed = _packed(sat, imgs)
    batch = ops.images_to_input(packed, Lb.IMG_NCHW, F32, size=case.out).cpu()
    batch_s2d = ops.images_to_input(packed, Lb.IMG_S2D16, BF, size=case.out).cpu() if name == "deep" else None
    assert {IC.taps([s], case.out) for s in case.sizes} != {IC.taps(case.sizes, case.out)}
    for b, img in enumerate(imgs):
        one = _packed(sat, [img])
        got = ops.images_to_input(one, Lb.IMG_NCHW, F32, size=case.out)
        assert same_bits(got, batch[b:b + 1]) and same_bits(got, ref[b:b + 1]), (b, img.shape)
        if batch_s2d is not None:
            got = ops.images_to_input(one, Lb.IMG_S2D16, BF, size=case.out)
            assert same_bits(got, batch_s2d[b:b + 1]) and same_bits(got, s2d16_of(ref[b:b + 1], BF)), (b, img.shape)


# ---------------------------------------------------------------------------- the layout kernels themselves
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 3, 10, 6), (1, 3, 224, 224), (2, 1, 8, 8)], ids=str)
def test_layout_kernels_equal_torch(sat, shape, dt):
    """ops.nchw_to_nhwc / ops.nchw_to_s2d (every kernel behind them: the 16-byte and the scalar NHWC stores, the
    generic S2D16 kernel and its RGB bf16 form) against permute / reshape / zero padding."""
    from sat_amd import ops
    x = torch.from_numpy(np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32))
    xd = x.to(DEV)
    for c_pad in (3, 8, 64):
        assert same_bits(ops.nchw_to_nhwc(xd, c_pad, dt), nhwc_of(x, c_pad, dt)), c_pad
    assert same_bits(ops.nchw_to_nhwc(xd, 4, F32), nhwc_of(x, 4, F32))   # the fp32 16-byte store
    assert same_bits(ops.nchw_to_s2d(xd, dt), s2d16_of(x, dt))


# ---------------------------------------------------------------------------- refusals: none reaches a launch
def _raw_call(sat, packed, size, layout, dtype, c_pad):
    """sat_images_to_input itself, past the checks of ops.images_to_input: (return code, the output buffer)."""
    from sat_amd import _lib as Lb
    lib = Lb.lib()
    OH, OW = size
    out = torch.full((packed.count * max(3, c_pad, 16) * OH * OW,), 7.0, device=DEV, dtype=dtype)
    ws_bytes = lib.sat_images_workspace_bytes(packed.count, OH, OW)
    ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
    m, sd = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    code = lib.sat_images_to_input(Lb.ptr(packed.pixels), Lb.ptr(packed.offsets), Lb.ptr(packed.sizes), packed.count,
                                   packed.max_h, packed.max_w, OH, OW, m, sd, layout, c_pad, Lb.dtype_code(dtype),
                                   Lb.ptr(out), Lb.ptr(ws), ws_bytes, Lb.stream_of(out))
    torch.cuda.synchronize()
    return code, out


@pytest.mark.parametrize("case", IC.REFUSED, ids=[c.name for c in IC.REFUSED])
def test_over_the_lds_limit_is_refused(sat, case):
    """More LDS than a workgroup can have: ValueError naming the limit from ops, SAT_ERR_INVALID from the entry point
    itself, and the output untouched -- no launch is attempted."""
    from sat_amd import ops, _lib as Lb
    lib = Lb.lib()
    packed = _packed(sat, [np.zeros(s + (3,), np.uint8) for s in case.sizes])
    need = lib.sat_images_lds_bytes(packed.max_h, packed.max_w, *case.out)
    limit = lib.sat_images_lds_limit()
    assert need == IC.lds_bytes(case.sizes, case.out) and limit == IC.LDS_LIMIT < need
    for layout, dt in ((Lb.IMG_NCHW, F32), (Lb.IMG_NHWC, BF), (Lb.IMG_S2D16, BF)):
        with pytest.raises(ValueError, match=f"{need} bytes of LDS.*{limit}"):
            ops.images_to_input(packed, layout, dt, size=case.out)
        code, out = _raw_call(sat, packed, case.out, layout, dt, 8)
        assert code == 9001 and bool((out == 7.0).all())


def test_fitting_lds_is_what_the_library_reports(sat):
    from sat_amd import _lib as Lb
    lib = Lb.lib()
    for case in IC.GPU_CASES:
        mh, mw = max(h for h, _ in case.sizes), max(w for _, w in case.sizes)
        assert lib.sat_images_lds_bytes(mh, mw, *case.out) == IC.lds_bytes(case.sizes, case.out) <= lib.sat_images_lds_limit()


def test_invalid_arguments_are_refused(sat):
    from sat_amd import ops, _lib as Lb
    packed = _packed(sat, [np.zeros((20, 30, 3), np.uint8)])
    with pytest.raises(RuntimeError, match=INVALID):                       # wider than MAX_OW
        ops.images_to_input(packed, Lb.IMG_NCHW, F32, size=(16, 513))
    for size in ((33, 17), (16, 17), (17, 16)):                             # S2D16 needs even sizes
        with pytest.raises(RuntimeError, match=INVALID):
            ops.images_to_input(packed, Lb.IMG_S2D16, BF, size=size)
    with pytest.raises(TypeError):                                          # NCHW is the reference's fp32 tensor
        ops.images_to_input(packed, Lb.IMG_NCHW, BF, size=(16, 16))
    for c_pad in (2, 65):
        for dt in (BF, F32):
            with pytest.raises(RuntimeError, match=INVALID):
                ops.images_to_input(packed, Lb.IMG_NHWC, dt, c_pad=c_pad, size=(16, 16))
    assert _raw_call(sat, packed, (16, 16), Lb.IMG_NCHW, BF, 8)[0] == 9001   # ... and the entry point itself
    code, out = _raw_call(sat, packed, (16, 513), Lb.IMG_NCHW, F32, 8)
    assert code == 9001 and bool((out == 7.0).all())

"""The decoder instance sat_decoder_instance reports (host code: csrc/decoder.hip splits_for, csrc/attention.hip
sat_attention_bwd_chunks) for every (family, B, dtype) of tests/test_gpu_batch_classes.py, without a GPU.

The GPU cases exist to cross the batch-size switches of the per-step kernels; a later change of a threshold would
leave them passing on another class than the one they are there for.  The values pinned here are derived by hand from
the code, with the transposed weight copies present as the Python layout always has them in bf16:

  pick_splits(M, N, K): tiles = cdiv(M, 128) cdiv(N, 64); want = cdiv(192, tiles); the largest divisor of K / 64 that
  is <= want; with none above 1 and K >= 1024, cdiv(kt, cdiv(kt, clamp(want, 2, 8))) ragged slabs.
  sat_skinny_splits(M, N, K) = K / 256 for M <= 128, N % 32 == 0, K % 256 == 0, K >= 1024, else 0 (not eligible).

  family R / G (D 2048, E 512, KH = 5 E + D = 4608)
    h      K = 512 < 1024: the tile kernel.  tiles = 72 (B <= 128) / 144, want 3 / 2, kt = 8              -> 2 / 2
    ctx    K = 2048: skinny 8 slabs, 512-deep pairs -> 4; B = 129: tiles 64, want 3, kt = 32              -> 4 / 2
    dgated K = 2048, transposed: skinny 8 -> 4; B = 129: tiles 2 x 32 = 64, want 3                        -> 4 / 2
    dh     K = 4608, transposed: skinny 18 -> 9, then the K >= 4096 rule: the largest c in (9, 16] with 36 % c == 0,
           16 c <= 256, 4608 / c <= 1024 -> 12; B = 129: tiles 16, want 12, kt = 72 -> 12, the rule finds no larger
                                                                                                           -> 12 / 12
  family V (D 512, E 512, KH = 3072)
    h      K = 512: tiles 48 / 96, want 4 / 2, kt = 8                                                     -> 4 / 2
    ctx    K = 512 < 1024: the tile kernel.  tiles 32 / 64, want 6 / 3, kt = 8                            -> 4 / 2
    dgated K = 2048, transposed: skinny 8 -> 4; B = 129: tiles 2 x 8 = 16, want 12, kt = 32               -> 4 / 8
    dh     K = 3072, transposed: skinny 12 -> 6 (K < 4096: no 12-slab rule); B = 129: want 12, kt = 48    -> 6 / 12
  family S (D 64, E 512, KH = 2624, B = 520: cdiv(B, 128) = 5)
    h      K = 512: tiles 5 x 41 = 205, want 1                                                            -> 1
    ctx    K = 64: one k-tile                                                                             -> 1
    dgated K = 2048: tiles 5 x 1, want 39 clamped to 32, kt = 32                                          -> 32
    dh     K = 2624 = 41 x 64 (prime): no divisor; K >= 1024: tiles 40, want 5, cdiv(41, cdiv(41, 5) = 9) -> 5

fp32 keeps a single split everywhere.  Attention-backward chunks: min(cdiv(256, B), cdiv(L, 4), 16).
"""
import ctypes

import pytest

# family: (D, L, E, V, T, tf, ado, batch sizes)
FAMILIES = {
    "R": (2048, 49, 512, 1003, 4, True, True, (1, 17, 33, 65, 127, 129)),
    "V": (512, 196, 512, 1000, 4, True, False, (1, 33, 129)),
    "G": (2048, 49, 512, 1003, 5, False, True, (33, 128, 129)),
    "S": (64, 16, 512, 120, 3, True, True, (520,)),
}

# (family, B): (h, ctx, dgated, dh) in bf16
BF16_SPLITS = {}
for _b in FAMILIES["R"][7]:
    BF16_SPLITS["R", _b] = (2, 4, 4, 12) if _b <= 128 else (2, 2, 2, 12)
for _b in FAMILIES["G"][7]:
    BF16_SPLITS["G", _b] = (2, 4, 4, 12) if _b <= 128 else (2, 2, 2, 12)
for _b in FAMILIES["V"][7]:
    BF16_SPLITS["V", _b] = (4, 4, 4, 6) if _b <= 128 else (2, 2, 8, 12)
BF16_SPLITS["S", 520] = (1, 1, 32, 5)

CHUNKS = {("R", 1): 13, ("R", 17): 13, ("R", 33): 8, ("R", 65): 4, ("R", 127): 3, ("R", 129): 2,
          ("V", 1): 16, ("V", 33): 8, ("V", 129): 2,
          ("G", 33): 8, ("G", 128): 2, ("G", 129): 2,
          ("S", 520): 1}

CASES = [(f, b) for f, spec in FAMILIES.items() for b in spec[7]]


@pytest.fixture(scope="module")
def lib():
    from sat_amd import _lib
    return _lib


def instance(L, family, B, bf16):
    D, Lf, E, V, T, tf, ado, _ = FAMILIES[family]
    d = L.SatDecoderDims()
    d.B, d.L, d.D, d.E, d.V, d.T = B, Lf, D, E, V, T
    d.tf, d.ado, d.attention, d.bert, d.training = int(tf), int(ado), 1, 0, 1
    d.dtype = L.SAT_BF16 if bf16 else L.SAT_F32
    d.has_dropout_mask = 1
    d.split_target = 0
    lay = L.SatDecoderLayout()
    for n in L.LAYOUT_FIELDS:
        setattr(lay, n, -1)
    if bf16:   # the transposed copies behind the bf16 shadow (Decoder._lp_t_offsets): only their presence counts here
        lay.wih_ctx_t, lay.hcat_t = 0, D * 4 * E
    out = (ctypes.c_int * 8)()
    L.check(L.lib().sat_decoder_instance(ctypes.byref(d), ctypes.byref(lay), out, 8), "sat_decoder_instance")
    return list(out)


def test_cases_are_those_of_the_gpu_file():
    """The GPU file builds its cases from its own table: the two must list the same (family, B)."""
    import test_gpu_batch_classes as gpu
    assert gpu.FAMILIES == FAMILIES
    assert gpu.CHUNKS == CHUNKS


@pytest.mark.parametrize("family,B", CASES, ids=[f"{f}{b}" for f, b in CASES])
def test_bf16_instance(lib, family, B):
    h, c, g, dh, chunks, tr, fwd, bwd = instance(lib, family, B, True)
    assert (h, c, g, dh) == BF16_SPLITS[family, B]
    assert chunks == CHUNKS[family, B]
    assert tr == 1
    assert (fwd, bwd) == (4, 4)


@pytest.mark.parametrize("family,B", CASES, ids=[f"{f}{b}" for f, b in CASES])
def test_fp32_instance(lib, family, B):
    """fp32 (parity mode): one split everywhere, no transposed copies, and the same chunks -- at D = 2048 too, where
    launch_bwd_split<float> takes dch = 8, ech = 2 (the one-launch attention backward, not the two-launch form)."""
    h, c, g, dh, chunks, tr, fwd, bwd = instance(lib, family, B, False)
    assert (h, c, g, dh) == (1, 1, 1, 1)
    assert chunks == CHUNKS[family, B]
    assert tr == 0
    assert (fwd, bwd) == (4, 4)


def test_skinny_and_tile_counts_differ_across_128(lib):
    """What the GPU file asserts between B = 127 and B = 129: the context product leaves the skinny kernel's count (4)
    for the tile kernel's pick_splits count (2)."""
    assert instance(lib, "R", 127, True)[1] != instance(lib, "R", 129, True)[1]
    assert instance(lib, "R", 128, True)[:4] == instance(lib, "R", 127, True)[:4]

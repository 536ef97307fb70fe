"""The sample-mode forward without a GPU: the entries are declared, exported and bound and refuse bad arguments before
any launch, and the host restatement of the noise (tests/sample_host.py, which the GPU tests compare the kernels with) is
exact in u, float64 in G and collision-free over the index ranges in use."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import sample_host as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 0x123456789ABCDEF, (1 << 64) - 1)


def test_entries_are_declared_exported_and_bound():
    import sat_amd
    L = sat_amd._lib
    header = open(os.path.join(REPO, "include", "sat_hip.h")).read()
    for name in ("sat_decoder_forward_sample", "sat_sample_noise", "sat_caption_loss_weighted_forward",
                 "sat_caption_loss_weighted_backward", "sat_caption_loss_weighted_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.EXPORTED and hasattr(L.lib(), name), name
    fn = L.lib().sat_decoder_forward_sample
    assert len(fn.argtypes) == 16 and fn.argtypes[7] is L.c_float
    assert L.lib().sat_abi_version() == 9 and L.ABI_VERSION == 9   # entries only added
    src = open(os.path.join(REPO, "show-attend-and-tell_amd", "csrc", "sat_internal.h")).read()
    assert f"kSatSampleDomain = 0x{H.SAMPLE_DOMAIN:016X}ULL" in src   # the restatement's constant is the kernels'


def test_entry_refuses_bad_arguments_before_any_launch():
    import sat_amd
    L = sat_amd._lib
    d, lay = L.SatDecoderDims(), L.SatDecoderLayout()
    d.B, d.L, d.D, d.E, d.V, d.T = 2, 4, 8, 64, 16, 4
    sampled = (ctypes.c_int32 * 8)()   # never written: every call below is refused first

    def call(tau):
        return L.lib().sat_decoder_forward_sample(ctypes.byref(d), ctypes.byref(lay), None, None, None, None, None, tau,
                                                  None, None, 0, None, None, None, sampled, None)
    d.tf = 1
    assert call(1.0) == 9001          # teacher forcing is sat_decoder_forward's
    d.tf = 0
    for tau in (-0.01, -1.0, float("nan")):
        assert call(tau) == 9001
    assert call(1.0) == 9001          # null pointers
    assert L.lib().sat_sample_noise(ctypes.byref(d), 2, 3, 16, None, None) == 9001
    assert L.lib().sat_sample_noise(None, 2, 3, 16, None, None) == 9001


def test_python_surface_validates_on_the_host():
    import sat_amd
    dec = sat_amd.Decoder(50, 64, attention=True)
    assert dec.sample_temperature_tensor is None
    feats = torch.zeros(2, 4, 64)
    with pytest.raises(RuntimeError, match="HIP device"):
        dec.sample(feats, 4)
    for name in ("weighted_caption_loss", "scst_weights"):
        assert name in sat_amd.__all__ and hasattr(sat_amd, name)
    with pytest.raises(RuntimeError, match="HIP device"):
        sat_amd.weighted_caption_loss(torch.zeros(2, 3, 5), torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32),
                                      torch.zeros(2, 3))


def test_u_is_exact_and_inside_the_open_interval():
    for seed in SEEDS:
        k = H.host_sample_k(seed, 5, 7, 1003)
        assert k.dtype == np.uint64 and int(k.max()) < (1 << 23)
        u = H.host_sample_uniform(seed, 5, 7, 1003)
        assert u.dtype == np.float64
        assert (u > 0).all() and (u < 1).all()
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)   # exact in fp32
        # exactly 24 significant bits: u 2^24 is an odd integer below 2^24
        m = u * 16777216.0
        assert np.array_equal(m, np.floor(m)) and (m.astype(np.int64) % 2 == 1).all() and (m < 16777216.0).all()
        g = H.host_sample_gumbel(seed, 5, 7, 1003)
        assert g.dtype == np.float64 and np.isfinite(g).all()
    # the ends of the range: k = 0 and k = 2^23 - 1 give finite noise of either sign
    lo, hi = 1.0 / 16777216.0, 1.0 - 1.0 / 16777216.0
    assert math.isfinite(-math.log(-math.log(lo))) and -math.log(-math.log(lo)) < 0
    assert math.isfinite(-math.log(-math.log(hi))) and -math.log(-math.log(hi)) > 16


def test_domain_constants_differ():
    assert len({H.SAMPLE_DOMAIN, H.TF_DOMAIN, H.DROPOUT_DOMAIN}) == 3
    src = open(os.path.join(REPO, "show-attend-and-tell_amd", "csrc", "sat_internal.h")).read()
    assert f"kSatTfDomain = 0x{H.TF_DOMAIN:016X}ULL" in src


def test_index_packing_does_not_collide():
    """(b, t, v) -> the packed word is injective over B <= 128, T <= 64, V <= 30522 (each index in a bit range of its
    own: v < 2^20, t < 2^20 above it, b from bit 40), and the mixed words of a block are distinct."""
    B, T, V = 128, 64, 30522
    assert V < (1 << 20) and T < (1 << 20) and B < (1 << 24)
    b = np.arange(B, dtype=np.uint64)
    t = np.arange(T, dtype=np.uint64)
    v = np.arange(V, dtype=np.uint64)
    # the three fields occupy disjoint bits, so XOR is concatenation
    assert int((b << np.uint64(40)).min(initial=1 << 63, where=b > 0)) > int((t << np.uint64(20)).max())
    assert int((t << np.uint64(20)).min(initial=1 << 63, where=t > 0)) > int(v.max())
    packed, mixed = H.host_sample_words(SEEDS[2], 4, T, V)          # 4 x 64 x 30522 = 7.8 M words
    assert np.unique(packed).size == packed.size
    assert np.unique(mixed).size == mixed.size                      # the mix is a bijection of the packed word + constant
    # the corners of the full range
    corner, _ = H.host_sample_words(SEEDS[2], B, 2, 2)
    assert int(corner[B - 1, 1, 1]) == ((B - 1) << 40) | (1 << 20) | 1
    full = ((np.uint64(B - 1) << np.uint64(40)) ^ (np.uint64(T - 1) << np.uint64(20)) ^ np.uint64(V - 1))
    assert int(full) == ((B - 1) << 40) | ((T - 1) << 20) | (V - 1)


def test_noise_is_gumbel_distributed():
    """A sanity check of the restatement itself: mean = Euler's constant, variance = pi^2 / 6 over 1.2 M values."""
    g = H.host_sample_gumbel(20170712, 8, 5, 30522)
    n = g.size
    sd = math.pi / math.sqrt(6.0)
    assert abs(g.mean() - 0.5772156649) <= 5 * sd / math.sqrt(n), g.mean()
    assert abs(g.var() - sd * sd) <= 0.02
    other = H.host_sample_gumbel(H.step_seed(20170712, 1), 8, 5, 30522)
    assert (other != g).mean() > 0.99   # the next counter value is another draw

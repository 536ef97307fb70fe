"""Host restatement of the sample-mode forward's noise (csrc/sat_internal.h sat_sample_gumbel), for the CPU and GPU
tests of sat_decoder_forward_sample and sat_sample_noise.

G[b, t, v] = -log(-log u) with u = (2k + 1) 2^-24, k = the top 23 bits of the 64-bit mix scheduled sampling's draw uses
(sched_sampling_host._mix64), taken over (seed ^ domain, b, t, v) under a domain constant of its own.  u is exact (24
significant bits, in the open interval (0, 1)); G is formed in float64.  ``seed`` is the decoder's ``_seed_host`` XOR the
device counter's term (sched_sampling_host.step_seed).
"""
import numpy as np

from sched_sampling_host import GOLDEN, M64, TF_DOMAIN, _mix64, step_seed  # noqa: F401  (step_seed: re-exported)

SAMPLE_DOMAIN = 0x3C6EF372FE94F82B
DROPOUT_DOMAIN = 0   # the dropout bit mixes the bare seed (csrc/lstm.hip dropout_keep)


def host_sample_words(seed, B, T1, V):
    """The packed index word ((b << 40) ^ (t << 20) ^ v) and the mixed 64-bit word, uint64 [B, T1, V]."""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    t = np.arange(T1, dtype=np.uint64)[None, :, None]
    v = np.arange(V, dtype=np.uint64)[None, None, :]
    packed = (b << np.uint64(40)) ^ (t << np.uint64(20)) ^ v
    with np.errstate(over="ignore"):
        x = np.uint64((int(seed) ^ SAMPLE_DOMAIN) & M64) * np.uint64(GOLDEN) + packed
        x = _mix64(x)
    return packed, x


def host_sample_k(seed, B, T1, V):
    """k: the top 23 bits of the mixed word, uint64 [B, T1, V]."""
    return host_sample_words(seed, B, T1, V)[1] >> np.uint64(41)


def host_sample_uniform(seed, B, T1, V):
    """u = (2k + 1) 2^-24 as float64 (exactly representable in float32), [B, T1, V]."""
    k = host_sample_k(seed, B, T1, V)
    return (2.0 * k.astype(np.float64) + 1.0) * (1.0 / 16777216.0)


def host_sample_gumbel(seed, B, T1, V):
    """G = -log(-log u), float64 [B, T1, V]."""
    return -np.log(-np.log(host_sample_uniform(seed, B, T1, V)))

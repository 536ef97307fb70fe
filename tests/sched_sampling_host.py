"""Host restatement of scheduled sampling's keep draw (csrc/sat_internal.h sat_tf_uniform, csrc/decoder.hip
tf_prefill_kernel), for the CPU and GPU tests of sat_decoder_forward_sampled.

keep[b, t] = u(seed, b, t) < p with u = the top 24 bits of a 64-bit mix of (seed ^ domain, b, t), scaled to [0, 1): a
function of (seed, b, t) only, under a domain constant of its own (the dropout bit of the same (b, t) is another
stream).  ``seed`` is the decoder's ``_seed_host`` XOR the device counter's term: counter 0 leaves it unchanged.
"""
import numpy as np

TF_DOMAIN = 0x7F4A7C15F39CC060
GOLDEN = 0x9E3779B97F4A7C15
COUNTER_MUL = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1


def _mix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    x = x ^ (x >> np.uint64(33))
    return x


def step_seed(seed_host, counter):
    """The seed of the forward whose device counter reads ``counter`` (SatDecoderDims.seed ^ f(*seed_ptr))."""
    return (int(seed_host) ^ ((int(counter) * COUNTER_MUL) & M64)) & M64


def host_tf_uniform(seed, B, T1):
    """u[b, t] in [0, 1), float32 (exact: 24 bits), for b < B, t < T1."""
    b = np.arange(B, dtype=np.uint64)[:, None]
    t = np.arange(T1, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = np.uint64((int(seed) ^ TF_DOMAIN) & M64) * np.uint64(GOLDEN) + ((b << np.uint64(40)) ^ (t << np.uint64(20)))
        x = _mix64(x)
    top = ((x & np.uint64(0xffffffff)) >> np.uint64(8)).astype(np.float32)
    return top * np.float32(1.0 / 16777216.0)


def host_tf_mask(seed, B, T1, p):
    """The keep mask [B, T1] uint8 a sampled forward reports for probability ``p``: column 0 (the start token) is 1."""
    keep = (host_tf_uniform(seed, B, T1) < np.float32(p)).astype(np.uint8)
    keep[:, 0] = 1
    return keep

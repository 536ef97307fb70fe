"""CIDEr-D resident on the device: the reward of self-critical sequence training without a host round
trip.

``CiderDDevice(cider, device)`` takes a host ``CiderD`` -- the specification, and the source of the document
frequencies -- and builds, once per corpus, what ``sat_cider_score`` reads: the stripped reference words with their
lengths, a CSR from image to references, an open-addressed hash table from n-gram to idf (the full 96-bit key and the
fp32 value per 16-byte slot) and the references' norms.  ``score(tokens, images)`` is then one launch on token matrices
that never leave the device; it reads nothing back and can be captured in a graph.
"""
import math

import numpy as np
import torch

from . import ops

MAX_WORDS = ops.CIDER_MAX_WORDS
ID_LIMIT = ops.CIDER_ID_LIMIT
SLOT_BYTES = 16


def pack_keys(ngrams):
    """The table's key words of n-grams (tuples of 1..4 ids below 2^20) as uint32 [n, 3] (include/sat_hip.h):
    word 0 = n << 20 | g0, word 1 = g1 | (g2 & 0xfff) << 20, word 2 = g2 >> 12 | g3 << 8."""
    ngrams = list(ngrams)
    ids = np.zeros((len(ngrams), 4), dtype=np.int64)
    n = np.zeros(len(ngrams), dtype=np.int64)
    for i, g in enumerate(ngrams):
        if not 1 <= len(g) <= 4:
            raise ValueError(f"pack_keys: an n-gram has 1 to 4 ids, got {len(g)}")
        n[i] = len(g)
        ids[i, :len(g)] = g
    if ids.size and (ids.min() < 0 or ids.max() >= ID_LIMIT):
        raise ValueError(f"pack_keys: ids must lie in [0, {ID_LIMIT})")
    out = np.empty((len(ngrams), 3), dtype=np.uint32)
    out[:, 0] = (n << 20) | ids[:, 0]
    out[:, 1] = ids[:, 1] | ((ids[:, 2] & 0xfff) << 20)
    out[:, 2] = (ids[:, 2] >> 12) | (ids[:, 3] << 8)
    return out


def keys_tensor(ngrams, device):
    """pack_keys as the int32 [n, 3] device tensor (the same bits) the ops take."""
    return torch.from_numpy(pack_keys(ngrams).view(np.int32)).to(device)


def default_table_slots(n_keys):
    """The smallest power of two that holds ``n_keys`` at a load of at most 50 %."""
    return max(16, 1 << (2 * max(1, n_keys) - 1).bit_length())


class CiderDDevice:
    """``CiderDDevice(cider, device, table_slots=None)``; ``score(tokens, images)``: tokens int32 [n, T1 <= 64] and
    images int64 [n] on the device -> float32 [n] on the device.  ``n_bad`` (one int32 on the device) counts the rows
    whose image index lay outside the corpus (they score 0); ``check_bad_images()`` reads it."""

    def __init__(self, cider, device, table_slots=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("CiderDDevice: the device must be a HIP device")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.cider, self.device, self.ids = cider, device, tuple(int(i) for i in cider.ids)
        refs = [r for refs in cider.refs for r in refs]
        longest = max((len(r) for r in refs), default=0)
        if longest > MAX_WORDS:
            raise ValueError(f"CiderDDevice: a reference has {longest} words; the device scorer takes at most "
                             f"{MAX_WORDS}")
        if any(t < 0 or t >= ID_LIMIT for r in refs for t in r):
            raise ValueError(f"CiderDDevice: reference ids must lie in [0, {ID_LIMIT})")
        self.n_images, self.n_refs = len(cider.refs), len(refs)
        stride = max(1, longest)
        words = np.zeros((max(1, len(refs)), stride), dtype=np.int32)
        lens = np.zeros(max(1, len(refs)), dtype=np.int32)
        for i, r in enumerate(refs):
            words[i, :len(r)] = r
            lens[i] = len(r)
        begin = np.zeros(self.n_images + 1, dtype=np.int64)
        np.cumsum([len(r) for r in cider.refs], out=begin[1:])
        if begin[-1] >= 1 << 31:
            raise ValueError("CiderDDevice: too many references")

        grams = list(cider.df)
        self.n_keys = len(grams)
        if table_slots is None:
            table_slots = default_table_slots(self.n_keys)
        table_slots = int(table_slots)
        if table_slots <= self.n_keys or table_slots < 2 or table_slots >= 1 << 31:
            raise ValueError(f"CiderDDevice: table_slots = {table_slots} must exceed the {self.n_keys} distinct "
                             "n-grams (one slot stays empty so that a probe ends), be at least 2 and below 2^31")
        self.table_slots = table_slots
        # idf in fp64 as CiderD._vec writes it (math.log, once per distinct df), rounded to fp32 once
        df = np.fromiter((cider.df[g] for g in grams), dtype=np.int64, count=len(grams))
        idf_of = {int(d): cider.log_n - math.log(max(1, int(d))) for d in np.unique(df)}
        values = np.array([idf_of[int(d)] for d in df], dtype=np.float64).astype(np.float32)
        self.log_n = float(np.float32(cider.log_n))

        self.ref_words = torch.from_numpy(words).to(device)
        self.ref_len = torch.from_numpy(lens[:len(refs)].copy()).to(device)
        self.img_ref_begin = torch.from_numpy(begin.astype(np.int32)).to(device)
        self.ref_norm = torch.zeros(max(1, len(refs)), 4, dtype=torch.float32, device=device)
        self.table = torch.zeros(table_slots, 4, dtype=torch.int32, device=device)
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=device)
        if grams:
            ops.cider_table_insert(self.table, keys_tensor(grams, device), torch.from_numpy(values).to(device),
                                   self.n_bad)
        bad = int(self.n_bad.item())   # the one sync of the build
        if bad:
            raise RuntimeError(f"CiderDDevice: {bad} of {self.n_keys} n-grams found no slot in a table of "
                               f"{table_slots}")
        ops.cider_ref_norms(self.table, self.log_n, self.ref_words, self.ref_len, self.ref_norm)

    @property
    def nbytes(self):
        """Bytes of HBM the resident corpus takes: the table, the references, their norms and the CSR."""
        ts = (self.table, self.ref_words, self.ref_len, self.ref_norm, self.img_ref_begin)
        return sum(t.numel() * t.element_size() for t in ts)

    @property
    def table_bytes(self):
        return self.table_slots * SLOT_BYTES

    def lookup(self, ngrams):
        """The stored idf of every n-gram (fp32 [n], device), log N for one the corpus does not hold."""
        return ops.cider_lookup(self.table, self.log_n, keys_tensor(ngrams, self.device))

    def score(self, tokens, images, out=None):
        for name, t, dtype, dim in (("tokens", tokens, torch.int32, 2), ("images", images, torch.int64, 1)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dim:
                raise ValueError(f"CiderDDevice.score: {name} must be a {dtype} tensor of {dim} dimension(s)")
            if t.device != self.device:
                raise ValueError(f"CiderDDevice.score: {name} lives on {t.device}, the corpus on {self.device}")
        if not 1 <= tokens.shape[1] <= MAX_WORDS:
            raise ValueError(f"CiderDDevice.score: tokens has {tokens.shape[1]} columns; the device scorer takes 1 to "
                             f"{MAX_WORDS}")
        if images.shape[0] != tokens.shape[0]:
            raise ValueError(f"CiderDDevice.score: {tokens.shape[0]} rows of tokens, {images.shape[0]} image indices")
        return ops.cider_score(self.table, self.log_n, self.ref_words, self.ref_len, self.ref_norm,
                               self.img_ref_begin, tokens.contiguous(), images.contiguous(), self.ids, out=out,
                               n_bad=self.n_bad)

    def check_bad_images(self):
        """Raise if any launch since the last check met an image index outside the corpus (one host sync)."""
        bad = int(self.n_bad.item())
        if bad:
            self.n_bad.zero_()
            raise RuntimeError(f"CiderDDevice: {bad} rows named an image outside [0, {self.n_images})")

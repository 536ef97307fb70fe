"""The frozen trunk's output per image, computed once and kept in HBM.

The dataset has one row per (image, caption) pair (dataset.py:15-52 repeats the image path per caption), so an epoch
over COCO pushes every image through the trunk five times, and the frozen trunk gives the same bits each time.
``FeatureCache`` assigns one slot per unique image key, fills a ``[n_images, row_elems]`` table on the device in one
pass over the unique images, and hands a training step its rows with one ``ops.rows_gather`` launch:

    cache = FeatureCache(encoder, dataset_keys, dtype, batch_size)
    cache.fill(cache.image_loader(dataset))          # or cache.load(dir, split)
    feats = cache.gather(cache.slots[dataset_rows])  # [n, *row_shape]

The cached tensor is ``encoder(imgs, dtype, steps=(0, encoder.tail_start()))``: the features ``[L, D]`` per image for
a frozen encoder, the NHWC activation entering the trainable tail for a fine-tuned one (the step then runs
``encoder(act, steps=(tail_start, len))``).  The fill always encodes full batches of ``batch_size`` -- the last one
padded by repeating its last image, the padded rows not stored -- so a cached row comes from the same kernel
instances as the row a full training batch of that size would compute.

The file layer (``table_key`` / ``write_table`` / ``read_table``) works on CPU tensors too.
"""
import hashlib
import json
import os

import numpy as np
import torch

from . import ops
from .data import PackedImages

# Bytes of HBM a table must leave free for the training step itself.  The default step's peak
# (torch.cuda.max_memory_allocated() of train.py's uncached loop at B = 128, V = 10000, T = 27, bf16) is 1.87 GB with
# ResNet152 and 2.46 GB with VGG19 (profiles/feature_cache/step_memory.json); this is 3.5 times the
# larger figure, which also covers the allocator's cached blocks and the batches in flight.
RESERVE_BYTES = 8 << 30

IO_CHUNK_BYTES = 256 << 20   # rows move between the device table and the file in pieces of at most this size
_DTYPE_NAMES = {torch.bfloat16: "bf16", torch.float32: "fp32"}


def _prefix_tensors(encoder):
    """(name, tensor) of every parameter and buffer outside the encoder's trainable tail, in state_dict order."""
    tail = {id(t) for t in encoder._tail_tensors()}
    named = list(encoder.net.named_parameters()) + list(encoder.net.named_buffers())
    return [(n, t) for n, t in named if id(t) not in tail]


def table_key(encoder, keys, dtype, row_shape, preprocess):
    """SHA-256 (hex) over everything a cached row depends on: the network, the dtype, ``tail_start()``, the row
    shape, the ordered key list, the preprocessing mode and the bytes of every prefix parameter and buffer.  The
    tail's weights are not part of it: a cached activation enters the tail, it does not depend on it."""
    h = hashlib.sha256()
    head = {"network": encoder.network, "dtype": _DTYPE_NAMES[dtype], "tail_start": encoder.tail_start(),
            "row_shape": [int(d) for d in row_shape], "preprocess": str(preprocess), "keys": [str(k) for k in keys]}
    h.update(json.dumps(head, sort_keys=True).encode())
    for name, t in _prefix_tensors(encoder):
        h.update(name.encode())
        h.update(t.detach().cpu().reshape(-1).view(torch.uint8).numpy().tobytes())   # reshape: BN's 0-dim counters
    return h.hexdigest()


def _paths(directory, split):
    return os.path.join(directory, f"features_{split}.bin"), os.path.join(directory, f"features_{split}.json")


def _row_chunk(table):
    return max(1, IO_CHUNK_BYTES // max(1, table.shape[1] * table.element_size()))


def write_table(directory, split, table, key, row_shape):
    """``table`` [n, row_elems] (any device) as a raw file plus a JSON sidecar naming its key, moved in chunks."""
    os.makedirs(directory, exist_ok=True)
    raw, side = _paths(directory, split)
    step = _row_chunk(table)
    with open(raw + ".tmp", "wb") as f:
        for i in range(0, table.shape[0], step):
            f.write(table[i:i + step].cpu().contiguous().view(torch.uint8).numpy().tobytes())
    os.replace(raw + ".tmp", raw)
    meta = {"key": key, "images": int(table.shape[0]), "row_shape": [int(d) for d in row_shape],
            "dtype": _DTYPE_NAMES[table.dtype], "bytes": table.numel() * table.element_size()}
    with open(side + ".tmp", "w") as f:
        json.dump(meta, f)
    os.replace(side + ".tmp", side)   # the sidecar last: a file without one reads as missing
    return meta


def read_sidecar(directory, split):
    """The sidecar's dict, or None when it or the raw file is missing or unreadable."""
    raw, side = _paths(directory, split)
    try:
        with open(side) as f:
            meta = json.load(f)
        meta["file_bytes"] = os.path.getsize(raw)
        return meta if isinstance(meta.get("row_shape"), list) else None
    except (OSError, ValueError, AttributeError):
        return None


def read_table(directory, split, table, key, row_shape):
    """Fill ``table`` [n, row_elems] (any device) from the file written under ``key``; False -- the caller rebuilds --
    when the sidecar or the file is missing, the key, the shape or the dtype differ, or the file is short."""
    meta = read_sidecar(directory, split)
    nbytes = table.numel() * table.element_size()
    if meta is None or meta.get("key") != key or meta.get("images") != table.shape[0] \
            or meta.get("row_shape") != [int(d) for d in row_shape] or meta.get("dtype") != _DTYPE_NAMES[table.dtype] \
            or meta.get("bytes") != nbytes or meta["file_bytes"] != nbytes:
        return False
    step = _row_chunk(table)
    row_bytes = table.shape[1] * table.element_size()
    with open(_paths(directory, split)[0], "rb") as f:
        for i in range(0, table.shape[0], step):
            rows = min(step, table.shape[0] - i)
            buf = np.fromfile(f, dtype=np.uint8, count=rows * row_bytes)
            if buf.size != rows * row_bytes:
                return False
            table[i:i + rows].copy_(torch.from_numpy(buf).view(table.dtype).view(rows, table.shape[1]))
    return True


class FeatureCache:
    def __init__(self, encoder, keys, dtype, batch_size):
        if dtype not in _DTYPE_NAMES:
            raise TypeError(f"FeatureCache: unsupported dtype {dtype} (float32 or bfloat16)")
        if batch_size <= 0:
            raise ValueError("FeatureCache: batch_size must be positive")
        self.encoder, self.dtype, self.batch_size = encoder, dtype, int(batch_size)
        slot_of, slots, first = {}, [], []
        for row, k in enumerate(keys):   # slots in order of first occurrence
            s = slot_of.get(k)
            if s is None:
                s = slot_of[k] = len(slot_of)
                first.append(row)
            slots.append(s)
        if not slots:
            raise ValueError("FeatureCache: no keys")
        self.slots = torch.tensor(slots, dtype=torch.int64)
        self.keys = list(slot_of)       # the unique keys, by slot
        self.first_rows = first         # the first dataset row of every slot: the rows a fill reads
        self.n_images = len(first)
        self.table = None               # [n_images, row_elems] on the device
        self.row_shape = None
        self.n_bad = None               # one int32 on the device: rows a launch found outside the table
        self._stamp = None              # (prefix state key, tail_start, dtype) at fill time

    # ---- sizes ----------------------------------------------------------------
    @staticmethod
    def required_bytes(n_images, row_shape, dtype, device=None):
        """Bytes of a table of ``n_images`` rows.  With ``device`` it also refuses a table that would leave less than
        RESERVE_BYTES of that device's memory free."""
        need = int(n_images) * int(np.prod([int(d) for d in row_shape], dtype=np.int64)) \
            * torch.empty((), dtype=dtype).element_size()
        if device is not None:
            free = torch.cuda.mem_get_info(device)[0]
            if need + RESERVE_BYTES > free:
                raise RuntimeError(f"FeatureCache: the table needs {need} bytes and the device has {free} bytes "
                                   f"free, which would leave less than the {RESERVE_BYTES} bytes reserved for the "
                                   "training step")
        return need

    def fill_plan(self):
        """The fill's batches: (slots encoded, how many of them are stored).  Every batch has ``batch_size`` images;
        the last one repeats its last image and stores only the real ones."""
        plan = []
        for s0 in range(0, self.n_images, self.batch_size):
            real = list(range(s0, min(s0 + self.batch_size, self.n_images)))
            plan.append((real + [real[-1]] * (self.batch_size - len(real)), len(real)))
        return plan

    def _allocate(self, row_shape, device):
        need = self.required_bytes(self.n_images, row_shape, self.dtype, device)
        try:
            table = torch.empty(self.n_images, int(np.prod([int(d) for d in row_shape], dtype=np.int64)),
                                device=device, dtype=self.dtype)
        except RuntimeError as e:   # torch.cuda.OutOfMemoryError is one
            raise RuntimeError(f"FeatureCache: allocating the table failed: it needs {need} bytes and the device "
                               f"has {torch.cuda.mem_get_info(device)[0]} bytes free") from e
        self.table, self.row_shape = table, tuple(int(d) for d in row_shape)
        if self.n_bad is None or self.n_bad.device != table.device:
            self.n_bad = torch.zeros(1, dtype=torch.int32, device=device)

    def _stamp_now(self, device):
        return (self.encoder._state_key(device, self.dtype), self.encoder.tail_start(), self.dtype)

    # ---- fill -----------------------------------------------------------------
    def image_loader(self, dataset, workers=0, collate_fn=None):
        """A loader over the first dataset row of every slot, in slot order, in batches of ``batch_size``.  It owns its
        generator: iterating it draws nothing from the global torch RNG, so a cached run shuffles as an uncached one."""
        return torch.utils.data.DataLoader(torch.utils.data.Subset(dataset, self.first_rows),
                                           batch_size=self.batch_size, shuffle=False, num_workers=workers,
                                           pin_memory=True, drop_last=False, collate_fn=collate_fn,
                                           generator=torch.Generator().manual_seed(0))

    @staticmethod
    def _pad(imgs, n):
        """``imgs`` with its last image repeated up to ``n`` images."""
        b = len(imgs)
        if isinstance(imgs, PackedImages):   # the pixels once, the last image's offset and size repeated
            return PackedImages(imgs.pixels, torch.cat([imgs.offsets, imgs.offsets[-1:].expand(n - b)]),
                                torch.cat([imgs.sizes, imgs.sizes[-1:].expand(n - b, 2)]), imgs.max_h, imgs.max_w)
        return torch.cat([imgs, imgs[-1:].expand(n - b, *imgs.shape[1:])])

    def fill(self, loader, device=None):
        """Encode the unique images (``loader`` yields them in slot order as fill_plan() batches them, ``batch_size``
        at a time and the rest last, as the batch or its first element) and scatter their rows into the table."""
        enc = self.encoder
        device = torch.device(device) if device is not None else next(enc.parameters()).device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        k, batches = enc.tail_start(), iter(loader)
        with torch.no_grad():
            for slots, real in self.fill_plan():
                batch = next(batches, None)
                imgs = batch[0] if isinstance(batch, (tuple, list)) else batch
                if imgs is None or len(imgs) != real:
                    raise ValueError(f"FeatureCache.fill: expected {real} images for slots {slots[0]}.., got "
                                     f"{'none' if imgs is None else len(imgs)} (batch_size {self.batch_size})")
                imgs = imgs.to(device, non_blocking=True)
                if real < len(slots):
                    imgs = self._pad(imgs, len(slots))
                act = enc(imgs, dtype=self.dtype, steps=(0, k))
                if slots[0] == 0 and (self.table is None or self.row_shape != tuple(act.shape[1:])
                                      or self.table.device != device):
                    self.table = None
                    self._allocate(act.shape[1:], device)
                idx = torch.arange(slots[0], slots[0] + real, device=device, dtype=torch.int64)
                ops.rows_scatter(act.reshape(len(slots), -1)[:real], idx, self.table, self.n_bad)
        if next(batches, None) is not None:
            raise ValueError(f"FeatureCache.fill: the loader gave more than {self.n_images} images")
        self.check_bad_rows()
        self._stamp = self._stamp_now(self.table.device)
        return self

    # ---- use ------------------------------------------------------------------
    def gather(self, slot_batch):
        """The rows of ``slot_batch`` (int64, host or device; they come from the sampler, so they are checked on the
        host when they live there) as a fresh [n, *row_shape] tensor, by one launch on the current stream."""
        if self.table is None or self._stamp is None:
            raise RuntimeError("FeatureCache.gather: the cache is empty (fill or load it first)")
        if self._stamp != self._stamp_now(self.table.device):
            raise RuntimeError("FeatureCache.gather: the encoder's frozen prefix, its tail_start() or the dtype changed "
                               "since the cache was filled; the cached rows are stale")
        slot_batch = torch.as_tensor(slot_batch, dtype=torch.int64)
        if slot_batch.dim() != 1:
            raise ValueError("FeatureCache.gather: slots must be a vector")
        if slot_batch.device.type == "cpu":
            if slot_batch.numel() and (int(slot_batch.min()) < 0 or int(slot_batch.max()) >= self.n_images):
                raise IndexError(f"FeatureCache.gather: slot outside [0, {self.n_images})")
            slot_batch = slot_batch.to(self.table.device, non_blocking=True)
        out = ops.rows_gather(self.table, slot_batch.contiguous(), n_bad=self.n_bad)
        return out.view((out.shape[0],) + self.row_shape)

    def check_bad_rows(self):
        """Raise if any launch since the last check met an index outside the table (one host sync: per epoch)."""
        if self.n_bad is not None:
            bad = int(self.n_bad.item())
            if bad:
                self.n_bad.zero_()
                raise RuntimeError(f"FeatureCache: {bad} rows were addressed outside the table")

    @property
    def nbytes(self):
        return 0 if self.table is None else self.table.numel() * self.table.element_size()

    # ---- files ----------------------------------------------------------------
    def save(self, directory, split, preprocess=""):
        key = table_key(self.encoder, self.keys, self.dtype, self.row_shape, preprocess)
        return write_table(directory, split, self.table, key, self.row_shape)

    def load(self, directory, split, preprocess="", device=None):
        """True when a valid file for this encoder prefix, key list, dtype and preprocessing was loaded; False (the
        cache left empty) when the caller has to fill."""
        meta = read_sidecar(directory, split)
        if meta is None:
            return False
        row_shape = tuple(int(d) for d in meta["row_shape"])
        key = table_key(self.encoder, self.keys, self.dtype, row_shape, preprocess)
        if meta.get("key") != key:   # before any allocation
            return False
        device = torch.device(device) if device is not None else next(self.encoder.parameters()).device
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.table = None
        self._allocate(row_shape, device)
        if not read_table(directory, split, self.table, key, row_shape):
            self.table = self.row_shape = self._stamp = None
            return False
        self._stamp = self._stamp_now(self.table.device)
        return True

"""The feature cache on the GPU.

Kernels (csrc/rows.hip): sat_rows_gather is bit-equal to torch.index_select and sat_rows_scatter is its inverse, for
both dtypes, for rows of 1 .. 100352 elements (the 16-B vector path and the element path, one chunk and many), with
either tensor starting one element off alignment, for 1 .. 128 rows, with canaries around everything written; bad
indices give zero rows / skipped rows and are counted; rows past 2 GiB and 4 GiB of a 4.84 GB table are addressed
right; a captured gather follows its index buffer.

FeatureCache: a gathered row is bit-equal to the row the encoder computes in a full batch, at every batch position,
also through a fine-tuned tail and its backward; a changed prefix weight makes the cache stale, a changed tail weight
does not.  train.py --cache-features / --feature-cache trains and evaluates to the same bits as the uncached run.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 64   # elements before and after every tensor a kernel writes (a multiple of 16 B in both dtypes)
ROW_ELEMS = [1, 7, 8, 1000, 100352]
NS = [1, 5, 128]
N_ROWS = 131


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _values(n, dtype, seed):
    """n distinct-looking finite values of ``dtype`` on the device (never the canary, never zero)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) + 1.0).to(dtype).to(DEV)


def _framed(rows, row_elems, dtype, off, fill=None):
    """A [rows, row_elems] view starting ``off`` elements past an aligned address, with CANARY elements of -7 on both
    sides -> (the whole buffer, the view)."""
    buf = torch.full((off + CANARY + rows * row_elems + CANARY,), -7.0, dtype=dtype, device=DEV)
    view = buf[off + CANARY: off + CANARY + rows * row_elems].view(rows, row_elems)
    assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
    if fill is not None:
        view.copy_(fill.view(rows, row_elems))
    return buf, view


def _frame_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    hi = lo + view.numel()
    return bool((buf[:lo] == -7).all()) and bool((buf[hi:] == -7).all())


@pytest.mark.parametrize("offs", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=["aligned", "both-off", "out-off", "table-off"])
@pytest.mark.parametrize("row_elems", ROW_ELEMS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_gather_is_index_select_and_scatter_its_inverse(sat, dtype, row_elems, offs):
    off_t, off_o = offs
    tbuf, table = _framed(N_ROWS, row_elems, dtype, off_t, _values(N_ROWS * row_elems, dtype, row_elems))
    before = table.clone()
    g = torch.Generator().manual_seed(row_elems + 17 * off_t + 31 * off_o)
    for n in NS:
        # gather: repeated and unsorted indices, first and last row among them
        idx = torch.randint(0, N_ROWS, (n,), generator=g)
        idx[0] = N_ROWS - 1
        if n > 2:
            idx[1], idx[2], idx[-1] = 0, N_ROWS - 1, 0
        idx = idx.to(DEV)
        obuf, out = _framed(n, row_elems, dtype, off_o)
        n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert sat.ops.rows_gather(table, idx, out=out, n_bad=n_bad) is out
        assert _same(out, torch.index_select(table, 0, idx))
        assert _frame_intact(obuf, out) and _frame_intact(tbuf, table) and _same(table, before)
        assert int(n_bad) == 0
        fresh = sat.ops.rows_gather(table, idx)   # allocates its output
        assert _same(fresh, out)
        # scatter: distinct indices; it undoes the gather of the same rows, and touches no other row
        perm = torch.randperm(N_ROWS, generator=g)[:n].to(DEV)
        src = torch.index_select(table, 0, perm)
        sbuf, target = _framed(N_ROWS, row_elems, dtype, off_o)
        sat.ops.rows_scatter(src, perm, target, n_bad)
        expect = torch.full_like(target, -7.0)
        expect[perm] = src
        assert _same(target, expect) and _frame_intact(sbuf, target)
        assert _same(sat.ops.rows_gather(target, perm), src)
        assert int(n_bad) == 0


@pytest.mark.parametrize("row_elems", [7, 1000, 100352])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_bad_indices_give_zero_rows_are_skipped_and_counted(sat, dtype, row_elems):
    n_rows = 9
    tbuf, table = _framed(n_rows, row_elems, dtype, 0, _values(n_rows * row_elems, dtype, 5))
    before = table.clone()
    idx = torch.tensor([3, -1, 8, n_rows, 0, -1, 5], dtype=torch.int64, device=DEV)
    good = (idx >= 0) & (idx < n_rows)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    obuf, out = _framed(idx.numel(), row_elems, dtype, 0)
    sat.ops.rows_gather(table, idx, out=out, n_bad=n_bad)
    assert int(n_bad) == 3
    assert _same(out[good], before[idx[good]]) and bool((out[~good] == 0).all())
    assert _frame_intact(obuf, out) and _frame_intact(tbuf, table) and _same(table, before)
    sat.ops.rows_gather(table, idx, out=out)   # without a counter: the same rows
    assert bool((out[~good] == 0).all()) and _same(out[good], before[idx[good]])
    # scatter: rows 3, 8, 0, 5 are written, the three bad ones skipped and counted on top of the gather's
    src = _values(idx.numel() * row_elems, dtype, 6).view(idx.numel(), row_elems)
    sat.ops.rows_scatter(src, idx, table, n_bad)
    assert int(n_bad) == 6
    expect = before.clone()
    expect[idx[good]] = src[good]
    assert _same(table, expect) and _frame_intact(tbuf, table)


def test_rows_past_2_and_4_gib_are_addressed_right(sat):
    """A 4.84 GB table (never filled): row 10,700 starts past 2^31 bytes and row 21,400 past 2^32."""
    n_rows, row = 24_100, 100_352
    assert 10_700 * row * 2 > 1 << 31 > 10_699 * row * 2 and 21_400 * row * 2 > 1 << 32 > 21_399 * row * 2
    table = torch.empty(n_rows, row, dtype=torch.bfloat16, device=DEV)
    slots = [0, 10_700, 21_400, 24_099]
    neighbours = [1, 10_699, 10_701, 21_399, 21_401, 24_098]
    marks = {s: float(i + 2) for i, s in enumerate(neighbours)}
    for s, v in marks.items():
        table[s].fill_(v)
    src = _values(len(slots) * row, torch.bfloat16, 9).view(len(slots), row)
    idx = torch.tensor(slots, dtype=torch.int64, device=DEV)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    sat.ops.rows_scatter(src, idx, table, n_bad)
    for i, s in enumerate(slots):   # torch's own indexing reads what the kernel wrote where it should have
        assert _same(table[s], src[i]), s
    for s, v in marks.items():
        assert bool((table[s] == v).all()), s
    order = torch.tensor([21_400, 0, 24_099, 10_700, 10_699], dtype=torch.int64, device=DEV)
    got = sat.ops.rows_gather(table, order, n_bad=n_bad)
    assert _same(got[:4], src[[2, 0, 3, 1]]) and bool((got[4] == marks[10_699]).all())
    assert int(n_bad) == 0


def test_a_captured_gather_follows_its_index_buffer(sat):
    row = 1000
    table = _values(50 * row, torch.bfloat16, 11).view(50, row)
    idx = torch.tensor([4, 4, 49, 0, 17], dtype=torch.int64, device=DEV)
    out = torch.zeros(5, row, dtype=torch.bfloat16, device=DEV)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    sat.ops.rows_gather(table, idx, out=out, n_bad=n_bad)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sat.ops.rows_gather(table, idx, out=out, n_bad=n_bad)
    for new in ([1, 2, 3, 5, 8], [49, 48, 48, 0, 0], [7, -1, 50, 7, 7]):
        idx.copy_(torch.tensor(new, dtype=torch.int64))
        out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        for i, r in enumerate(new):
            assert _same(out[i], table[r] if 0 <= r < 50 else torch.zeros_like(out[i])), (new, i)
    assert int(n_bad) == 2


# =====================================================================================================================
# FeatureCache
# =====================================================================================================================
HW = 64            # 2 x 2 feature maps for ResNet152, 4 x 4 for VGG19
N_IMAGES, BATCH = 10, 4
# 25 dataset rows over 10 images; first occurrences are in the order 3, 0, 7, 1, 9, 4, 2, 8, 6, 5
ROW_IMAGE = [3, 0, 3, 7, 1, 9, 0, 4, 2, 2, 8, 6, 3, 5, 1, 7, 9, 9, 4, 0, 5, 6, 8, 2, 1]

_ENCODERS = {}


def _images():
    return torch.randn(N_IMAGES, 3, HW, HW, generator=torch.Generator().manual_seed(77))


def _encoder(sat, network, dtype, fine_tune=0):
    key = (network, dtype, fine_tune)
    if key not in _ENCODERS:
        torch.manual_seed(5)
        _ENCODERS[key] = sat.Encoder(network, dtype=dtype, fine_tune=fine_tune).to(DEV).eval()
    return _ENCODERS[key]


def _filled(sat, enc, dtype):
    cache = sat.FeatureCache(enc, [f"img{i}" for i in ROW_IMAGE], dtype, BATCH)
    assert cache.n_images == N_IMAGES and cache.keys[:4] == ["img3", "img0", "img7", "img1"]
    by_slot = _images()[[int(k[3:]) for k in cache.keys]]
    state = torch.get_rng_state()
    cache.fill([by_slot[i:i + BATCH] for i in range(0, N_IMAGES, BATCH)])   # 4 + 4 + 2: the last batch is padded
    assert torch.equal(torch.get_rng_state(), state)
    return cache


def _row_groups():
    """Batches of 4 dataset rows: consecutive ones, then the same rows at other batch positions and with repeats."""
    groups = [list(range(i, i + BATCH)) for i in range(0, len(ROW_IMAGE) - BATCH + 1, BATCH)]
    groups += [[24, 23, 22, 21], [13, 13, 20, 13], [5, 16, 17, 0]]
    return groups


@pytest.mark.parametrize("network,dtype", [("vgg19", torch.float32), ("vgg19", torch.bfloat16),
                                           ("resnet152", torch.bfloat16)], ids=["vgg19-fp32", "vgg19-bf16", "rn152-bf16"])
def test_cached_rows_are_the_encoders_rows_bit_for_bit(sat, network, dtype):
    enc = _encoder(sat, network, dtype)
    cache = _filled(sat, enc, dtype)
    L = (HW // 32) ** 2 if network == "resnet152" else (HW // 16) ** 2
    assert cache.row_shape == (L, enc.dim) and cache.table.shape == (N_IMAGES, L * enc.dim)
    assert cache.nbytes == sat.FeatureCache.required_bytes(N_IMAGES, cache.row_shape, dtype)
    images = _images()
    with torch.no_grad():
        for rows in _row_groups():
            ref = enc(images[[ROW_IMAGE[r] for r in rows]].to(DEV), dtype=dtype)
            got = cache.gather(cache.slots[rows])
            assert got.shape == ref.shape and got.dtype == dtype
            for pos in range(BATCH):
                assert _same(got[pos], ref[pos]), (rows, pos)
    cache.check_bad_rows()
    with pytest.raises(IndexError):
        cache.gather(torch.tensor([0, N_IMAGES]))
    with pytest.raises(IndexError):
        cache.gather(torch.tensor([-1]))


def test_cache_of_a_fine_tuned_encoder_feeds_its_tail_and_its_backward(sat):
    dtype = torch.bfloat16
    enc = _encoder(sat, "resnet152", dtype, fine_tune=1)
    cache = _filled(sat, enc, dtype)
    k, n = enc.tail_start(), enc._plan_len()
    assert k == n - 1 and cache.row_shape == (HW // 32, HW // 32, 2048)   # the NHWC activation entering the tail
    rows = [5, 16, 17, 0]
    imgs = _images()[[ROW_IMAGE[r] for r in rows]].to(DEV)
    d_feats = torch.randn(BATCH, (HW // 32) ** 2, 2048, generator=torch.Generator().manual_seed(8)).to(dtype).to(DEV)
    ref = enc(imgs, dtype=dtype)
    ref.backward(d_feats)
    ref_grads = enc.tail_grad_flat.clone()
    enc.tail_grad_flat.zero_()   # the attached views accumulate: start the second backward from zero
    got = enc(cache.gather(cache.slots[rows]), dtype=dtype, steps=(k, n))
    assert got.requires_grad and _same(got.detach(), ref.detach())
    got.backward(d_feats)
    assert bool(ref_grads.abs().sum() > 0) and torch.equal(enc.tail_grad_flat, ref_grads)
    with torch.no_grad():   # evaluation: the same tail without a graph
        assert _same(enc(cache.gather(cache.slots[rows]), dtype=dtype, steps=(k, n)), ref.detach())
    # staleness: a tail-only update keeps the cache valid, a prefix update does not
    with torch.no_grad():
        enc.net[7][2].conv1.weight.mul_(1.0)
    cache.gather(cache.slots[rows])
    with torch.no_grad():
        enc.net[0].weight.mul_(1.0)   # same values, another version: the key is the version, as for the plan
    with pytest.raises(RuntimeError, match="stale"):
        cache.gather(cache.slots[rows])
    _ENCODERS.pop(("resnet152", dtype, 1))


def test_cache_files_round_trip_through_the_device(sat, tmp_path):
    dtype = torch.bfloat16
    enc = _encoder(sat, "vgg19", dtype)
    cache = _filled(sat, enc, dtype)
    cache.save(str(tmp_path), "val", "synthetic")
    again = sat.FeatureCache(enc, [f"img{i}" for i in ROW_IMAGE], dtype, BATCH)
    assert not again.load(str(tmp_path), "train", "synthetic") and not again.load(str(tmp_path), "val", "host")
    assert again.load(str(tmp_path), "val", "synthetic")
    assert again.row_shape == cache.row_shape and _same(again.table, cache.table)
    assert _same(again.gather(again.slots[[3, 9, 24]]), cache.gather(cache.slots[[3, 9, 24]]))
    other = sat.FeatureCache(enc, [f"img{i}" for i in ROW_IMAGE[::-1]], dtype, BATCH)
    assert not other.load(str(tmp_path), "val", "synthetic") and other.table is None


# =====================================================================================================================
# train.py
# =====================================================================================================================
def _train_main(argv, capsys):
    spec = importlib.util.spec_from_file_location("sat_train_cli_fc_gpu",
                                                  os.path.join(REPO, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(argv)
    torch.cuda.synchronize()
    return [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]


def _scores(recs):
    return [{k: v for k, v in r.items() if k.startswith(("val_", "test_"))} for r in recs
            if any(k.startswith(("val_", "test_")) for k in r)]


def test_train_cli_from_the_cache_matches_the_uncached_run(sat, tmp_path, capsys):
    """Every val / test batch of this run is a full batch (16 images each), so the full-batch fill covers them."""
    base = ["--synthetic", "64", "--batch-size", "16", "--epochs", "2", "--max-steps", "2", "--network", "vgg19",
            "--tf", "--ado", "--attention", "--vocab", "300"]
    runs = {"plain": [], "cached": ["--cache-features"], "built": ["--feature-cache", str(tmp_path / "fc")],
            "loaded": ["--feature-cache", str(tmp_path / "fc")]}
    recs, ckpt = {}, {}
    for name, extra in runs.items():
        out = tmp_path / name
        recs[name] = _train_main(base + extra + ["--out", str(out)], capsys)
        ckpt[name] = torch.load(out / "model_vgg19_2.pth", weights_only=True, map_location="cpu")
    assert not [r for r in recs["plain"] if "feature_cache" in r]
    assert len(_scores(recs["plain"])) == 3   # val after each epoch, test at the end
    for name in ("cached", "built", "loaded"):
        how = [(r["feature_cache"], r["split"], r["images"]) for r in recs[name] if "feature_cache" in r]
        word = "loaded" if name == "loaded" else "built"
        assert how == [(word, "train", 64), (word, "val", 16), (word, "test", 16)], how
        assert all(r["bytes"] == r["images"] * 196 * 512 * 2 and r["seconds"] >= 0
                   for r in recs[name] if "feature_cache" in r)
        assert _scores(recs[name]) == _scores(recs["plain"]), name
        assert list(ckpt[name]) == list(ckpt["plain"])
        for k, v in ckpt["plain"].items():
            assert torch.equal(ckpt[name][k], v), (name, k)
    assert sorted(os.listdir(tmp_path / "fc")) == sorted(f"features_{s}.{e}" for s in ("train", "val", "test")
                                                         for e in ("bin", "json"))

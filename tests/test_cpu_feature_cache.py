"""The feature cache without a GPU: sat_rows_gather / sat_rows_scatter are exported, bound and refuse bad arguments
before any launch; FeatureCache assigns slots in order of first occurrence and plans full fill batches; the file layer
(raw file + JSON sidecar keyed by a SHA-256 over everything a cached row depends on) round-trips CPU tensors and reads
anything else as invalid; train.py takes the flags."""
import ctypes
import importlib.util
import os

import pytest
import torch

INVALID = 9001
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import sat_amd
    return sat_amd._lib


@pytest.fixture(scope="module")
def FC():
    import sat_amd.feature_cache as fc
    return fc


def test_entries_are_exported_and_bound(L):
    import sat_amd
    for name in ("sat_rows_gather", "sat_rows_scatter"):
        assert name in L.EXPORTED and hasattr(L.lib(), name)
    assert callable(sat_amd.ops.rows_gather) and callable(sat_amd.ops.rows_scatter)
    assert sat_amd.FeatureCache is sat_amd.feature_cache.FeatureCache and "FeatureCache" in sat_amd.__all__
    assert L.lib().sat_abi_version() == 9


def test_bad_arguments_are_refused_before_any_launch(L):
    ok = ctypes.c_void_p(1 << 20)   # never dereferenced: the argument checks come first
    g, s = L.lib().sat_rows_gather, L.lib().sat_rows_scatter
    # gather(table, n_rows, row_elems, dtype, idx, n, out, n_bad, stream)
    assert g(None, 4, 8, L.SAT_BF16, ok, 2, ok, None, None) == INVALID
    assert g(ok, 4, 8, L.SAT_BF16, None, 2, ok, None, None) == INVALID
    assert g(ok, 4, 8, L.SAT_BF16, ok, 2, None, None, None) == INVALID
    assert g(ok, 4, 8, L.SAT_BF16, ok, -1, ok, None, None) == INVALID
    assert g(ok, 0, 8, L.SAT_BF16, ok, 2, ok, None, None) == INVALID
    assert g(ok, -3, 8, L.SAT_BF16, ok, 2, ok, None, None) == INVALID
    assert g(ok, 4, 0, L.SAT_BF16, ok, 2, ok, None, None) == INVALID
    assert g(ok, 4, 8, 2, ok, 2, ok, None, None) == INVALID
    assert g(ok, 4, 8, -1, ok, 2, ok, None, None) == INVALID
    # scatter(src, n, row_elems, dtype, idx, table, n_rows, n_bad, stream)
    assert s(None, 2, 8, L.SAT_F32, ok, ok, 4, None, None) == INVALID
    assert s(ok, 2, 8, L.SAT_F32, None, ok, 4, None, None) == INVALID
    assert s(ok, 2, 8, L.SAT_F32, ok, None, 4, None, None) == INVALID
    assert s(ok, -1, 8, L.SAT_F32, ok, ok, 4, None, None) == INVALID
    assert s(ok, 2, 0, L.SAT_F32, ok, ok, 4, None, None) == INVALID
    assert s(ok, 2, 8, L.SAT_F32, ok, ok, 0, None, None) == INVALID
    assert s(ok, 2, 8, 5, ok, ok, 4, None, None) == INVALID
    # n == 0: success, nothing launched (there is no device here to launch on)
    for dt in (L.SAT_F32, L.SAT_BF16):
        assert g(ok, 4, 8, dt, ok, 0, ok, None, None) == 0
        assert s(ok, 0, 8, dt, ok, ok, 4, None, None) == 0
    assert g(ok, 4, 8, 7, ok, 0, ok, None, None) == INVALID   # ... but still checked


def test_ops_refuse_cpu_tensors():
    import sat_amd
    table, idx = torch.zeros(4, 8), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        sat_amd.ops.rows_gather(table, idx)
    with pytest.raises(RuntimeError, match="HIP device"):
        sat_amd.ops.rows_scatter(torch.zeros(2, 8), idx, table)


def test_slots_follow_first_occurrence_and_fill_batches_are_full():
    import sat_amd
    enc = sat_amd.Encoder("vgg19")
    cache = sat_amd.FeatureCache(enc, ["a", "b", "a", "c", "b", "a"], torch.bfloat16, 2)
    assert cache.slots.dtype == torch.int64 and cache.slots.tolist() == [0, 1, 0, 2, 1, 0]
    assert cache.n_images == 3 and cache.keys == ["a", "b", "c"] and cache.first_rows == [0, 1, 3]
    assert cache.fill_plan() == [([0, 1], 2), ([2, 2], 1)]   # the last batch repeats its last image, stores one row
    big = sat_amd.FeatureCache(enc, range(10), torch.float32, 4)   # SyntheticDataset's keys: the row index
    assert big.slots.tolist() == list(range(10)) and big.n_images == 10
    assert big.fill_plan() == [([0, 1, 2, 3], 4), ([4, 5, 6, 7], 4), ([8, 9, 9, 9], 2)]
    assert all(len(s) == 4 for s, _ in big.fill_plan())
    # the padding itself, on a host batch
    padded = sat_amd.FeatureCache._pad(torch.arange(2.0).view(2, 1, 1, 1).expand(2, 3, 2, 2), 4)
    assert padded.shape == (4, 3, 2, 2) and padded[:, 0, 0, 0].tolist() == [0.0, 1.0, 1.0, 1.0]
    packed = sat_amd.PackedImages.from_arrays([torch.zeros(2, 3, 3, dtype=torch.uint8),
                                               torch.ones(4, 2, 3, dtype=torch.uint8)])
    pp = sat_amd.FeatureCache._pad(packed, 4)
    assert len(pp) == 4 and pp.offsets.tolist() == [0, 18, 18, 18] and pp.sizes.tolist() == [[2, 3]] + [[4, 2]] * 3
    with pytest.raises(RuntimeError, match="empty"):
        cache.gather(torch.tensor([0]))


def test_required_bytes():
    import sat_amd
    need = sat_amd.FeatureCache.required_bytes(113287, (49, 2048), torch.bfloat16)
    assert need == 22_737_154_048 and isinstance(need, int)
    assert sat_amd.FeatureCache.required_bytes(113287, (49, 2048), torch.float32) == 2 * need
    assert sat_amd.FeatureCache.required_bytes(113287, (196, 512), torch.bfloat16) == need
    # at least twice the larger measured peak of the default step (VGG19, 2,462,141,440 bytes)
    assert sat_amd.feature_cache.RESERVE_BYTES >= 2 * 2_462_141_440


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_file_round_trip_and_invalidation(FC, tmp_path, dtype, monkeypatch):
    import sat_amd
    monkeypatch.setattr(FC, "IO_CHUNK_BYTES", 3 * 32 * dtype.itemsize)   # 3 rows per piece: 7 rows take 3 pieces
    torch.manual_seed(3)
    enc = sat_amd.Encoder("vgg19")
    keys, row_shape = [f"img{i}" for i in range(7)], (4, 8)
    table = torch.randn(7, 32).to(dtype)
    key = FC.table_key(enc, keys, dtype, row_shape, "host")
    meta = FC.write_table(str(tmp_path), "train", table, key, row_shape)
    assert meta["bytes"] == 7 * 32 * dtype.itemsize == os.path.getsize(tmp_path / "features_train.bin")
    back = torch.zeros_like(table)
    assert FC.read_table(str(tmp_path), "train", back, key, row_shape)
    assert torch.equal(back.view(torch.uint8), table.view(torch.uint8))
    # missing split, another key list, another order, another preprocessing mode, another dtype: invalid
    assert not FC.read_table(str(tmp_path), "val", back, key, row_shape)
    assert FC.table_key(enc, keys[:-1] + ["other"], dtype, row_shape, "host") != key
    assert FC.table_key(enc, keys[::-1], dtype, row_shape, "host") != key
    assert FC.table_key(enc, keys, dtype, row_shape, "device") != key
    assert FC.table_key(enc, keys, dtype, (8, 4), "host") != key
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    assert FC.table_key(enc, keys, other, row_shape, "host") != key
    assert not FC.read_table(str(tmp_path), "train", back, FC.table_key(enc, keys[::-1], dtype, row_shape, "host"),
                             row_shape)
    assert FC.table_key(enc, keys, dtype, row_shape, "host") == key   # and it is a function of its inputs only
    # one changed prefix weight element: another key, so the file reads as invalid
    with torch.no_grad():
        enc.net[0].weight[3, 1, 2, 0] += 1.0
    changed = FC.table_key(enc, keys, dtype, row_shape, "host")
    assert changed != key and not FC.read_table(str(tmp_path), "train", back, changed, row_shape)
    # a truncated file: invalid under its own key
    raw = tmp_path / "features_train.bin"
    data = raw.read_bytes()
    raw.write_bytes(data[:-1])
    assert not FC.read_table(str(tmp_path), "train", back, key, row_shape)
    raw.write_bytes(data)
    assert FC.read_table(str(tmp_path), "train", back, key, row_shape)
    os.remove(tmp_path / "features_train.json")
    assert not FC.read_table(str(tmp_path), "train", back, key, row_shape)


@pytest.mark.parametrize("network,tail_param", [("vgg19", "net.34.weight"), ("resnet152", "net.7.2.bn3.weight")])
def test_tail_weights_are_not_part_of_the_key(FC, network, tail_param):
    import sat_amd
    enc = sat_amd.Encoder(network, fine_tune=1)
    keys = list(range(5))
    key = FC.table_key(enc, keys, torch.bfloat16, (2, 2, 8), "synthetic")
    params = dict(enc.named_parameters())
    with torch.no_grad():
        params[tail_param].view(-1)[0] += 1.0   # a trainable tail weight: the cached activation does not depend on it
    assert FC.table_key(enc, keys, torch.bfloat16, (2, 2, 8), "synthetic") == key
    with torch.no_grad():
        next(iter(enc.net.parameters())).view(-1)[0] += 1.0   # the first conv: the prefix
    assert FC.table_key(enc, keys, torch.bfloat16, (2, 2, 8), "synthetic") != key
    frozen = sat_amd.Encoder(network)   # nothing trainable: another tail_start, and the tail's weights do count
    assert FC.table_key(frozen, keys, torch.bfloat16, (2, 2, 8), "synthetic") != key


def _train_module():
    spec = importlib.util.spec_from_file_location("sat_train_cli_fc",
                                                  os.path.join(REPO, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_flags_and_captions_only_datasets(tmp_path):
    T = _train_module()
    a = T.parse([])
    assert a.cache_features is False and a.feature_cache is None
    assert T.parse(["--cache-features"]).cache_features is True
    b = T.parse(["--feature-cache", str(tmp_path)])
    assert b.cache_features is True and b.feature_cache == str(tmp_path)
    assert "--cache-features" in T.__doc__ and "--feature-cache" in T.__doc__
    ds = T.SyntheticDataset(6, 50, 12, False, seed=1, captions_only=True)
    row, cap, all_caps = ds[4]
    assert row == 4 and torch.equal(cap, ds.caps[4]) and all_caps.shape == (1, 12)
    full = T.SyntheticDataset(6, 50, 12, False, seed=1)
    assert full[4][0].shape == (3, 224, 224) and torch.equal(full[4][1], cap)
    # the fill's loader yields the unique images in slot order and leaves the global torch RNG alone
    import sat_amd
    cache = sat_amd.FeatureCache(sat_amd.Encoder("vgg19"), [0, 1, 1, 2, 0, 3], torch.float32, 3)
    before = torch.get_rng_state()
    batches = [b[0] for b in cache.image_loader(full)]
    assert torch.equal(torch.get_rng_state(), before)
    assert [len(b) for b in batches] == [3, 1] and torch.equal(batches[0][2], full[3][0])
    args = T.parse(["--synthetic", "8", "--batch-size", "4", "--vocab", "50", "--seq", "12"])
    rows, caps, _ = next(iter(T.loaders(args, "val", 0, 1, captions_only=True)))
    assert rows.dtype == torch.int64 and rows.tolist() == [0, 1, 2, 3] and caps.shape == (4, 12)

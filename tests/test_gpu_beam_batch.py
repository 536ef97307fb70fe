"""Batched beam search (Decoder.caption_batch / sat_decoder_beam_search_batch) on the device.

fp32 mode is compared per image with ``oracle.beam_search`` on the fixtures of beam_batch_fixtures.py
(test_cpu_beam_batch_fixtures.py shows their top-k margins are far from rounding noise, so the ids
must be equal): ids bit-exact, alpha rows and the winning score within 1e-4 relative, the project's
fp32 parity bound (test_beam_search_matches_reference).  Every test here needs an MI355X."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import beam_batch_fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "show-attend-and-tell_amd")
PARITY_SETS = ("A", "B_ado", "B_noatt", "B_bert")


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


@pytest.fixture(scope="module")
def decoder_of(sat):
    cache = {}

    def get(name):
        if name not in cache:
            g, _ = FX.load(name)
            c, p = g["cfg"], g["params"]
            kw = dict(tf=False, ado=c["ado"], bert=c["bert"], attention=c["attention"])
            if c["bert"]:
                dec = sat.Decoder(c["V"], c["D"], bert_embedding_weight=p["embedding.weight"], **kw)
            else:
                dec = sat.Decoder(c["V"], c["D"], **kw)
            dec.load_state_dict(p, strict=True)
            cache[name] = dec.to(DEV).eval()
        return cache[name]
    return get


def rel(a, b):
    a = torch.as_tensor(np.asarray(a, dtype=np.float64)); b = torch.as_tensor(np.asarray(b, dtype=np.float64))
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def check_against(got, want, tag):
    """got: caption_batch tuples; want: oracle tuples (ids, alphas, score)."""
    assert len(got) == len(want)
    for i, ((ids, al, score), (e_ids, e_al, e_score)) in enumerate(zip(got, want)):
        assert ids == e_ids, (tag, i)
        al = np.asarray(al, dtype=np.float64)
        assert al.shape == e_al.shape, (tag, i)
        assert rel(al, e_al) < 1e-4, (tag, i)
        if math.isinf(e_score):
            assert math.isinf(score) and score < 0, (tag, i)
        else:
            assert abs(score - e_score) <= 1e-4 * max(1.0, abs(e_score)), (tag, i)


def same_ids_close_scores(got, want, tag):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0], (tag, i)
        if math.isinf(b[2]):
            assert math.isinf(a[2])
        else:
            assert abs(a[2] - b[2]) <= 1e-4 * max(1.0, abs(b[2])), (tag, i)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_step", FX.MAX_STEPS)
@pytest.mark.parametrize("name", PARITY_SETS)
def test_fp32_matches_oracle(decoder_of, name, max_step):
    g, feats = FX.load(name)
    got = decoder_of(name).caption_batch(feats.to(DEV), g["cfg"]["beam"], max_step=max_step)
    check_against(got, FX.expected(name, max_step), (name, max_step))


# 2 ---------------------------------------------------------------------------------------------
def test_fp32_matches_single_image_path(decoder_of):
    g, feats = FX.load("A")
    R, dec = g["cfg"]["beam"], decoder_of("A")
    f = feats.to(DEV)
    got = dec.caption_batch(f, R)
    for i in range(f.shape[0]):
        ids, _ = dec.caption(f[i:i + 1].expand(R, f.shape[1], f.shape[2]), R)
        assert got[i][0] == ids, i


# 3 ---------------------------------------------------------------------------------------------
def test_batch_composition_invariance(decoder_of):
    """An image's result does not depend on its neighbours (scores within 1e-4, not bitwise: the GEMM
    launcher picks its form by the row count)."""
    g, feats = FX.load("A")
    R, dec = g["cfg"]["beam"], decoder_of("A")
    f = feats.to(DEV)
    base = dec.caption_batch(f, R)
    perm = [4, 0, 6, 2, 5, 1, 3]
    got = dec.caption_batch(f[perm].contiguous(), R)
    same_ids_close_scores(got, [base[j] for j in perm], "permuted")
    got = dec.caption_batch(f[:1], R) + dec.caption_batch(f[1:], R)
    same_ids_close_scores(got, base, "1 + 6")


# 4 ---------------------------------------------------------------------------------------------
def test_chunking(decoder_of):
    g, feats = FX.load("A")
    R, dec = g["cfg"]["beam"], decoder_of("A")
    f = feats.to(DEV)
    whole, chunks = dec.caption_batch(f, R, max_images=64), dec.caption_batch(f, R, max_images=3)
    assert len(chunks) == len(whole) == 7
    assert [c[0] for c in chunks] == [w[0] for w in whole]


def test_row_limit(decoder_of):
    """341 images x beam 3 = 1023 of the 1024 rows one call may carry (set A repeated): every copy of an image
    gives that image's oracle ids, wherever it sits in the batch."""
    g, feats = FX.load("A")
    R, dec = g["cfg"]["beam"], decoder_of("A")
    reps = feats.repeat(49, 1, 1)[:341].contiguous()
    got = dec.caption_batch(reps.to(DEV), R, max_step=6, max_images=341)
    want = FX.expected("A", 6)
    assert len(got) == 341
    same_ids_close_scores(got, [want[i % 7] for i in range(341)], "341 images")


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_step", FX.MAX_STEPS)
def test_beam_one_single_image(decoder_of, max_step):
    g, feats = FX.load("beam1")
    assert feats.shape[0] == 1 and g["cfg"]["beam"] == 1
    got = decoder_of("beam1").caption_batch(feats.to(DEV), 1, max_step=max_step)
    check_against(got, FX.expected("beam1", max_step), ("beam1", max_step))


# 6 ---------------------------------------------------------------------------------------------
def well_formed(out, beam, max_step, L, start=0):
    """No ids comparison in bf16: as test_beam_search_bf16_and_bench_shape notes, the margins are below
    bf16 noise."""
    n_none = 0
    for ids, al, score in out:
        al = torch.as_tensor(np.asarray(al, dtype=np.float32))
        assert al.shape[1] == L
        if math.isinf(score):
            n_none += 1
            assert ids == [0] and al.shape[0] == beam
            assert torch.allclose(al.sum(1), torch.ones(beam), atol=1e-3)
        else:
            assert ids[0] == start and 1 <= len(ids) <= max_step + 2 and al.shape[0] == len(ids)
            assert torch.allclose(al[1:].sum(1), torch.ones(len(ids) - 1), atol=1e-3)
    return n_none


@pytest.mark.parametrize("max_step", FX.MAX_STEPS)
def test_bf16_small_shape(decoder_of, max_step):
    g, feats = FX.load("A")
    c = g["cfg"]
    out = decoder_of("A").caption_batch(feats.to(DEV).bfloat16(), c["beam"], max_step=max_step)
    assert len(out) == 7
    well_formed(out, c["beam"], max_step, c["L"])


def test_bf16_coco_shape(sat):
    torch.manual_seed(0)
    V, D, L, N, R = 10000, 2048, 49, 8, 3
    dec = sat.Decoder(V, D, ado=True, attention=True).to(DEV).eval()
    feats = torch.randn(N, L, D, device=DEV).bfloat16()
    out = dec.caption_batch(feats, R)
    assert len(out) == N
    well_formed(out, R, 50, L)
    assert all(len(ids) <= 52 for ids, _, _ in out)


# 7 ---------------------------------------------------------------------------------------------
def test_argument_checks(sat, decoder_of):
    g, feats = FX.load("A")
    dec, L = decoder_of("A"), sat._lib
    f = feats.to(DEV)
    many = f[:1].expand(342, f.shape[1], f.shape[2]).contiguous()   # 342 * 3 = 1026 rows > 1024
    with pytest.raises(RuntimeError, match="caption_batch"):
        dec.caption_batch(many, 3, max_images=342)
    with pytest.raises(RuntimeError, match="caption_batch"):
        dec.caption_batch(f, 3, max_step=0)                          # beam 3 > max_step + 2
    with pytest.raises(ValueError, match=r"\[N, L, D\]"):
        dec.caption_batch(f[0], 3)                                   # wrong rank
    dims = dec._dims(f, torch.empty(1, 3, dtype=torch.long))
    size = L.lib().sat_decoder_beam_batch_workspace_bytes
    assert size(ctypes.byref(dims), 7, 3, 50) > 0
    assert size(ctypes.byref(dims), 341, 3, 50) > 0                  # 1023 rows: allowed
    assert size(ctypes.byref(dims), 342, 3, 50) == 0
    assert size(ctypes.byref(dims), 7, 3, 0) == 0
    assert size(ctypes.byref(dims), 0, 3, 50) == 0
    assert size(ctypes.byref(dims), 7, 0, 50) == 0
    # the entry itself refuses them too (before any launch: the workspace pointer is never touched)
    lay = dec._layout()
    ids = np.zeros(4, dtype=np.int32)
    code = L.lib().sat_decoder_beam_search_batch(ctypes.byref(dims), ctypes.byref(lay), L.ptr(dec._flat), None,
                                                 L.ptr(f), 7, 3, 0, None, 0, ids.ctypes.data, ids.ctypes.data,
                                                 ids.ctypes.data, ids.ctypes.data, ids.ctypes.data, L.stream_of(f))
    assert code != 0


# 8, 9 ------------------------------------------------------------------------------------------
def _train(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--synthetic", "32", "--batch-size", "16",
                        "--epochs", "1", "--max-steps", "1", "--network", "vgg19", "--ado", "--attention",
                        "--vocab", "200", "--out", str(out_dir), *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.fixture(scope="module")
def plain_run(sat, tmp_path_factory):
    out = tmp_path_factory.mktemp("plain")
    return out, _train(out)


def test_generate_caption_img_dir(plain_run, tmp_path):
    from PIL import Image
    out_dir, _ = plain_run
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for i in range(3):
        Image.fromarray((np.random.default_rng(i).random((120 + 10 * i, 150, 3)) * 255).astype(np.uint8)).save(
            imgs / f"im{i}.png")
    cli = [sys.executable, os.path.join(PKG, "generate_caption.py"), "--model", str(out_dir / "model_vgg19_1.pth")]
    r = subprocess.run(cli + ["--img-dir", str(imgs)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 3 and len({rec["path"] for rec in recs}) == 3
    assert all(rec["ids"][0] == 0 for rec in recs)
    r = subprocess.run(cli + ["--img-path", str(imgs / "im0.png")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(recs) == 1 and "path" not in recs[0] and set(recs[0]) == {"caption", "ids", "score"}


def test_train_beam_eval(plain_run, tmp_path):
    _, plain = plain_run
    recs = _train(tmp_path, "--beam-eval", "3")
    beam_keys = {f"val_beam_bleu{i}" for i in range(1, 5)}
    val = [r for r in recs if "val_bleu4" in r]
    assert len(val) == 1 and beam_keys <= set(val[0])
    for k in beam_keys:
        assert isinstance(val[0][k], float) and 0.0 <= val[0][k] <= 1.0
    plain_val = [r for r in plain if "val_bleu4" in r]
    assert len(plain_val) == 1
    assert set(plain_val[0]) == {"epoch", "val_loss", "val_top1_acc", "val_top5_acc", "val_bleu1", "val_bleu2",
                                 "val_bleu3", "val_bleu4"}
    assert set(val[0]) - beam_keys == set(plain_val[0])

"""Scheduled sampling without a GPU: sat_decoder_forward_sampled is declared, exported and bound; Decoder.tf_prob
validates; train.py's schedule and flags; CPU tensors are still refused; and the host restatement of the keep draw
(tests/sched_sampling_host.py, which the GPU test compares the kernels with) behaves like a Bernoulli(p) draw."""
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import sched_sampling_host as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _train_module():
    spec = importlib.util.spec_from_file_location("sat_train_cli_ss",
                                                  os.path.join(REPO, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_is_declared_exported_and_bound():
    import sat_amd
    L = sat_amd._lib
    header = open(os.path.join(REPO, "include", "sat_hip.h")).read()
    assert re.search(r"\bint\s+sat_decoder_forward_sampled\s*\(", header)
    assert "decoder.py:108-112" in header and "131-133" in header
    assert "sat_decoder_forward_sampled" in L.EXPORTED
    fn = L.lib().sat_decoder_forward_sampled
    assert len(fn.argtypes) == 17 and fn.argtypes[7] is L.c_float
    assert L.lib().sat_abi_version() == 9 and L.ABI_VERSION == 9
    assert "sat_decoder_forward_sampled" in open(os.path.join(REPO, "INTEGRATION.md")).read()


def test_entry_refuses_bad_arguments_before_any_launch():
    import ctypes
    import sat_amd
    L = sat_amd._lib
    d, lay = L.SatDecoderDims(), L.SatDecoderLayout()
    d.B, d.L, d.D, d.E, d.V, d.T = 2, 4, 8, 64, 16, 4
    call = lambda: L.lib().sat_decoder_forward_sampled(ctypes.byref(d), ctypes.byref(lay), None, None, None, None,  # noqa: E731
                                                       None, p, None, None, None, None, 0, None, None, None, None)
    p = 0.5
    d.tf = 1
    assert call() == 9001          # teacher forcing is sat_decoder_forward's
    d.tf = 0
    for p in (-0.01, 1.01, float("nan")):
        assert call() == 9001
    p = 0.5
    assert call() == 9001          # null pointers


def test_tf_prob_validation():
    import sat_amd
    dec = sat_amd.Decoder(50, 64, attention=True)
    assert dec.tf_prob is None and dec.tf_prob_tensor is None and dec.tf_mask is None and dec.last_tf_mask is None
    for ok in (0, 0.0, 0.25, 1, 1.0):
        dec.tf_prob = ok
        assert dec.tf_prob == float(ok) and isinstance(dec.tf_prob, float)
    dec.tf_prob = None
    assert dec.tf_prob is None
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "0.5", True, [0.5]):
        with pytest.raises(ValueError):
            dec.tf_prob = bad
    assert dec.tf_prob is None
    assert "tf_prob" not in dec.state_dict() and "_tf_prob" not in dec.state_dict()


def test_cpu_tensors_are_still_refused():
    import sat_amd
    dec = sat_amd.Decoder(50, 64, attention=True).train()
    dec.tf_prob = 0.5
    with pytest.raises(RuntimeError, match="HIP device"):
        dec(torch.zeros(2, 4, 64), torch.zeros(2, 5, dtype=torch.long))


def test_schedule():
    f = _train_module().tf_prob_schedule
    assert f(1, 10, 0.75, 0.25) == 0.75 and f(10, 10, 0.75, 0.25) == 0.25
    vals = [f(e, 10, 0.75, 0.25) for e in range(1, 11)]
    assert all(a > b for a, b in zip(vals, vals[1:]))
    assert all(math.isclose(a - b, 0.5 / 9, rel_tol=1e-9) for a, b in zip(vals, vals[1:]))   # linear
    up = [f(e, 4, 0.0, 1.0) for e in range(1, 5)]
    assert up == sorted(up) and up[0] == 0.0 and up[-1] == 1.0
    assert [f(e, 5, 0.5, 0.5) for e in range(1, 6)] == [0.5] * 5       # Q = P
    assert f(1, 1, 0.75, 0.25) == 0.75                                  # a single epoch trains at P
    assert f(1, 2, 0.75, 0.25) == 0.75 and f(2, 2, 0.75, 0.25) == 0.25
    assert all(0.0 <= f(e, 7, 1.0, 0.0) <= 1.0 for e in range(1, 8))


def test_train_flags_and_config_keys():
    T = _train_module()
    a = T.parse([])
    assert a.tf_prob is None and a.tf_prob_end is None
    b = T.parse(["--tf-prob", "0.75"])
    assert b.tf_prob == 0.75 and b.tf_prob_end == 0.75 and b.tf is False
    c = T.parse(["--synthetic", "64", "--tf-prob", "0.75", "--tf-prob-end", "0.25", "--epochs", "2", "--max-steps", "3",
                 "--tf", "--cache-features", "--fine-tune-encoder", "1"])
    assert (c.tf_prob, c.tf_prob_end, c.tf, c.cache_features, c.fine_tune_encoder) == (0.75, 0.25, True, True, 1)
    cfg = json.loads(json.dumps(dict(vars(c))))     # what main() writes into model_config.json
    assert cfg["tf_prob"] == 0.75 and cfg["tf_prob_end"] == 0.25
    assert set(vars(a)) == set(vars(c))             # additive keys, present (null) without the flag
    for bad in (["--tf-prob", "1.5"], ["--tf-prob", "-0.1"], ["--tf-prob", "0.5", "--tf-prob-end", "2"],
                ["--tf-prob-end", "0.5"]):
        with pytest.raises(SystemExit):
            T.parse(bad)
    assert "--tf-prob" in T.__doc__ and "--tf-prob-end" in T.__doc__


def test_host_draw_ends_are_exact():
    for seed in (0, 1, 0x123456789ABCDEF, (1 << 64) - 1):
        u = H.host_tf_uniform(seed, 64, 20)
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        assert not (u < np.float32(0.0)).any()      # p = 0 keeps none
        assert (u < np.float32(1.0)).all()          # p = 1 keeps all
        assert (H.host_tf_mask(seed, 64, 20, 0.0)[:, 1:] == 0).all()
        assert (H.host_tf_mask(seed, 64, 20, 1.0) == 1).all()
        assert (H.host_tf_mask(seed, 64, 20, 0.0)[:, 0] == 1).all()   # the start token's column is reported as kept


SEED = 20151113   # the draw below is a property of the restatement alone at this seed (checked here, on the CPU)


def test_host_draw_varies_and_meets_the_binomial_bound():
    B, T1, p = 64, 20, 0.25
    m = H.host_tf_mask(SEED, B, T1, p)[:, 1:]
    n = m.size
    assert n == 64 * 19
    # a Bernoulli(p) mean over n draws: 5 sigma = 5 sqrt(p (1 - p) / n) = 0.062
    bound = 5 * math.sqrt(p * (1 - p) / n)
    assert abs(bound - 0.062) < 1e-3
    assert abs(m.mean() - p) <= bound, m.mean()
    assert (m.std(axis=0) > 0).all()      # varies along b in every column
    assert (m.std(axis=1) > 0).sum() >= B - 1      # and along t (a row of 19 draws is constant with probability 0.4 %)
    rows = {r.tobytes() for r in m}
    cols = {c.tobytes() for c in m.T}
    assert len(rows) > B // 2 and len(cols) == T1 - 1
    # another seed, and another counter value of the same seed, are other draws
    assert (H.host_tf_mask(SEED + 1, B, T1, p) != H.host_tf_mask(SEED, B, T1, p)).any()
    assert H.step_seed(SEED, 0) == SEED and H.step_seed(SEED, 1) != SEED
    assert (H.host_tf_mask(H.step_seed(SEED, 1), B, T1, p) != H.host_tf_mask(SEED, B, T1, p)).any()


def test_host_draw_is_not_the_dropout_bit():
    """The domain constant: the keep draw at p = 0.5 is not the dropout bit of element 0 of the same (b, t)."""
    B, T1 = 64, 20
    with np.errstate(over="ignore"):
        b = np.arange(B, dtype=np.uint64)[:, None]
        t = np.arange(T1, dtype=np.uint64)[None, :]
        x = np.uint64(SEED) * np.uint64(H.GOLDEN) + ((b << np.uint64(40)) ^ (t << np.uint64(20)))
        drop = (H._mix64(x) & np.uint64(1)).astype(np.uint8)
    keep = (H.host_tf_uniform(SEED, B, T1) < np.float32(0.5)).astype(np.uint8)
    agree = (drop == keep).mean()
    assert abs(agree - 0.5) <= 5 * math.sqrt(0.25 / (B * T1)), agree

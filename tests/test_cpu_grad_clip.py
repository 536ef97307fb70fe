"""Gradient clipping by global norm without a GPU: the option's validation in ``sat_amd.Adam``, the
``--clip-grad-norm`` flag of train.py and the ops wrappers' refusal of CPU tensors."""
import importlib.util
import math
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sat():
    import sat_amd
    return sat_amd


@pytest.fixture(scope="module")
def train_cli():
    spec = importlib.util.spec_from_file_location("sat_train_cli_clip",
                                                  os.path.join(REPO, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _param():
    return [torch.zeros(3, requires_grad=True)]


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.0, math.nan, math.inf, -math.inf])
def test_adam_rejects_max_grad_norm(sat, bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        sat.Adam(_param(), max_grad_norm=bad)


def test_adam_max_grad_norm_default_and_value(sat):
    opt = sat.Adam(_param())
    assert opt.max_grad_norm is None
    assert opt.grad_norm is None and opt.clip_scale is None and opt.skipped_steps is None
    opt = sat.Adam(_param(), max_grad_norm=5)
    assert opt.max_grad_norm == 5.0 and isinstance(opt.max_grad_norm, float)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = 0.0
    assert opt.max_grad_norm == 5.0
    assert "bias corrections follow" in " ".join(sat.optim.__doc__.split())


def test_train_flag(train_cli):
    assert train_cli.parse([]).clip_grad_norm is None
    assert train_cli.parse(["--clip-grad-norm", "5"]).clip_grad_norm == 5.0
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            train_cli.parse(["--clip-grad-norm", bad])
    assert "--clip-grad-norm" in train_cli.__doc__


def test_ops_refuse_cpu_tensors(sat):
    g = torch.ones(8)
    with pytest.raises(RuntimeError, match="HIP device"):
        sat.ops.grad_sumsq(g, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HIP device"):
        sat.ops.grad_clip_finalize(torch.zeros(2, dtype=torch.float64), 1.0, torch.zeros(4))
    with pytest.raises(RuntimeError, match="HIP device"):
        sat.ops.adam_step_scaled_(g.clone(), g, g.clone(), g.clone(), None, 0.9, 0.999, 1e-8, 1e-3, 1.0,
                                  torch.zeros(4))


def test_partials_per_range(sat):
    """One workgroup per sweep of 4096 elements, at least 1, at most 1024."""
    f = sat.ops.grad_sumsq_partials
    assert [f(n) for n in (0, 1, 4096, 4097, 1024 * 4096, 10 ** 9)] == [1, 1, 1, 2, 1024, 1024]

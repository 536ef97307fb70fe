"""The host side of sat_conv3x3_wgrad (csrc/convwgrad.hip) without a GPU: the entry points exist, refuse what the
kernel does not run before anything is launched, and the workspace the planner asks for follows its split choice.
Then Encoder.fine_tune(n) (which parameters become trainable, tail_start(), the split state key, train.py's flags), the
fold's chain rule as pure torch against fp64 autograd, and the tail gradients' all-reduce over two gloo ranks."""
import ctypes

import pytest

INVALID = 9001
TICKET_BYTES = 256 * 4


@pytest.fixture(scope="module")
def L():
    import sat_amd
    return sat_amd._lib


def _ws(L, shape, split_k=0, dtype=None):
    N, H, W, Cin, Cout = shape
    pol = L.SatPolicy(split_k=split_k)
    return L.lib().sat_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout, L.SAT_BF16 if dtype is None else dtype,
                                                     ctypes.pointer(pol))


def test_entries_are_bound(L):
    assert "sat_conv3x3_wgrad" in L.EXPORTED and "sat_conv3x3_wgrad_workspace_bytes" in L.EXPORTED
    assert hasattr(L.lib(), "sat_conv3x3_wgrad")


@pytest.mark.parametrize("shape", [(1, 4, 4, 64, 128), (1, 4, 4, 128, 192), (1, 4, 4, 136, 128), (1, 4, 4, 0, 128),
                                   (0, 4, 4, 128, 128), (1, 0, 4, 128, 128), (1 << 14, 32, 32, 128, 128)])
def test_unsupported_shapes_are_refused_before_any_launch(L, shape):
    N, H, W, Cin, Cout = shape
    assert _ws(L, shape) == 0
    fake = ctypes.c_void_p(1 << 20)   # never dereferenced: the shape check comes first
    assert L.lib().sat_conv3x3_wgrad(N, H, W, Cin, Cout, L.SAT_BF16, fake, fake, fake, 0, None, 0, None, None) == INVALID


def test_fp32_needs_the_im2col_workspace(L):
    assert _ws(L, (2, 7, 7, 128, 128), dtype=L.SAT_F32) == 2 * 7 * 7 * 9 * 128 * 4
    fake = ctypes.c_void_p(1 << 20)
    assert L.lib().sat_conv3x3_wgrad(2, 7, 7, 128, 128, L.SAT_F32, fake, fake, fake, 0, None, 0, None, None) == INVALID
    assert L.lib().sat_conv3x3_wgrad(2, 7, 7, 128, 128, 7, fake, fake, fake, 0, None, 0, None, None) == INVALID


def test_null_and_unaligned_pointers_are_refused(L):
    ok, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)
    f = L.lib().sat_conv3x3_wgrad
    assert f(2, 7, 7, 128, 128, L.SAT_BF16, None, ok, ok, 0, None, 0, None, None) == INVALID
    assert f(2, 7, 7, 128, 128, L.SAT_BF16, ok, odd, ok, 0, None, 0, None, None) == INVALID
    assert f(2, 7, 7, 128, 128, L.SAT_BF16, ok, ok, odd, 0, None, 0, None, None) == INVALID


def test_workspace_follows_the_split_count(L):
    tile128 = 128 * 128 * 4
    # K = 147 pixels = 3 k-tiles, 9 output tiles of 128 x 128: a forced split count holds that many partials per tile
    assert _ws(L, (3, 7, 7, 128, 128), 1) == TICKET_BYTES
    assert _ws(L, (3, 7, 7, 128, 128), 2) == 2 * 9 * tile128 + TICKET_BYTES
    assert _ws(L, (3, 7, 7, 128, 128), 3) == 3 * 9 * tile128 + TICKET_BYTES
    # one k-tile cannot be split: a forced count the shape does not allow leaves the planner's choice
    assert _ws(L, (2, 2, 2, 128, 128), 3) == _ws(L, (2, 2, 2, 128, 128), 0) == TICKET_BYTES
    # the trunk's shapes at B = 128 (layer4's c2, VGG19 block 5): 72 tiles of 256 x 128, split; under the 32 MiB cap
    for shape in [(128, 7, 7, 512, 512), (128, 14, 14, 512, 512)]:
        ws = _ws(L, shape)
        assert (ws - TICKET_BYTES) % (72 * 2 * tile128) == 0 and 2 <= (ws - TICKET_BYTES) // (72 * 2 * tile128) <= 3, ws
        assert ws <= (32 << 20) + TICKET_BYTES


# =====================================================================================================================
# Encoder.fine_tune(n), the fold's chain rule, the tail gradients' all-reduce
# =====================================================================================================================
import os   # noqa: E402
import tempfile   # noqa: E402

import torch   # noqa: E402
import torch.nn.functional as F   # noqa: E402

RESNET_UNIT = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight",
               "bn3.weight", "bn3.bias")


def _expected(network, n):
    if network == "resnet152":
        return {f"net.7.{b}.{m}" for b in (2, 1)[:n] for m in RESNET_UNIT}
    return {f"net.{i}.{m}" for i in (34, 32, 30, 28)[:n] for m in ("weight", "bias")}


@pytest.fixture(scope="module")
def encoders():
    import sat_amd
    torch.manual_seed(0)
    return {net: sat_amd.Encoder(net) for net in ("resnet152", "vgg19")}


@pytest.mark.parametrize("network,limit", [("resnet152", 2), ("vgg19", 4)])
def test_fine_tune_marks_exactly_the_named_parameters(encoders, network, limit):
    import sat_amd
    enc = encoders[network]
    keys = list(enc.state_dict())
    frozen_plan_len = len(enc.compiled_plan(torch.device("cpu"), torch.float32))
    for n in list(range(limit + 1)) + [0]:
        assert enc.fine_tune(n) is enc
        got = {k for k, p in enc.named_parameters() if p.requires_grad}
        assert got == _expected(network, n), n
        assert [k for k, _ in enc.named_parameters() if k in got] == \
            [k for k, p in enc.named_parameters() if any(p is q for q in enc.tail_parameters())]
        assert list(enc.state_dict()) == keys                      # state-dict keys do not change
        assert enc.tail_start() == frozen_plan_len - n == enc._plan_len() - n
    for bad in (limit + 1, -1, 99):
        with pytest.raises(ValueError, match=str(limit)):
            enc.fine_tune(bad)
    assert {k for k, p in enc.named_parameters() if p.requires_grad} == set()   # a refused n changes nothing
    with pytest.raises(ValueError, match=str(limit)):
        sat_amd.Encoder(network, fine_tune=limit + 1)


def test_tail_start_points_at_the_units_plan_entries(encoders):
    enc = encoders["vgg19"].fine_tune(3)
    plan = enc.compiled_plan(torch.device("cpu"), torch.float32)
    k = enc.tail_start()
    assert [s[0] for s in plan[k:]] == ["conv"] * 3 and plan[k - 1][0] == "conv" and plan[k - 2][0] == "pool"
    assert plan[k][1][0].shape == (512, 3, 3, 512)
    enc.fine_tune(0)
    enc = encoders["resnet152"].fine_tune(2)
    plan = enc.compiled_plan(torch.device("cpu"), torch.float32)
    k = enc.tail_start()
    assert [s[0] for s in plan[k:]] == ["block", "block"] and all(s[4] is None for s in plan[k:])   # identity shortcuts
    assert plan[k - 1][4] is not None   # net.7.0 (projection, stride 2) stays out
    enc.fine_tune(0)


def test_prefix_key_ignores_the_tail_and_the_tail_key_sees_it(encoders):
    enc = encoders["vgg19"].fine_tune(2)
    dev = torch.device("cpu")
    k0, t0 = enc._state_key(dev, torch.float32), enc._tail_key()
    with torch.no_grad():
        enc.net[34].weight.mul_(1.0)
    assert enc._state_key(dev, torch.float32) == k0 and enc._tail_key() != t0
    with torch.no_grad():
        enc.net[28].weight.mul_(1.0)   # not in the tail at n = 2
    assert enc._state_key(dev, torch.float32) != k0
    enc.fine_tune(0)
    assert enc._tail_key() == ()


def test_train_parser_flags():
    import importlib.util
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sat_train_cli", os.path.join(repo, "show-attend-and-tell_amd", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse([])
    assert a.fine_tune_encoder == 0 and a.encoder_lr == 1e-5
    a = mod.parse(["--fine-tune-encoder", "2", "--encoder-lr", "3e-6"])
    assert a.fine_tune_encoder == 2 and a.encoder_lr == 3e-6


# ---- the fold's chain rule (the formula of sat_conv_fold_backward) against autograd, fp64 ----
def _fold_backward(dwf, dbf, w, gamma, mean, var, eps=1e-5):
    """dwf [Cout,KH,KW,Cin], dbf [Cout] -> (conv.weight.grad [Cout,Cin,KH,KW], bn.weight.grad, bn.bias.grad)"""
    rstd = 1.0 / torch.sqrt(var + eps)
    s = gamma * rstd
    gw = dwf.permute(0, 3, 1, 2) * s[:, None, None, None]
    gg = rstd * ((dwf.permute(0, 3, 1, 2) * w).sum(dim=(1, 2, 3)) - dbf * mean)
    return gw, gg, dbf


@pytest.mark.parametrize("k", [1, 3])
def test_fold_chain_rule_matches_autograd(k):
    from oracle import sat_oracle as O
    g = torch.Generator().manual_seed(7 + k)
    co, ci, n, hw = 6, 5, 3, 4
    x = torch.randn(n, ci, hw, hw, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    p = {"bn.weight": torch.rand(co, generator=g, dtype=torch.float64) + 0.5,
         "bn.bias": torch.randn(co, generator=g, dtype=torch.float64),
         "bn.running_mean": torch.randn(co, generator=g, dtype=torch.float64),
         "bn.running_var": torch.rand(co, generator=g, dtype=torch.float64) + 0.5}
    for t in ("bn.weight", "bn.bias"):
        p[t].requires_grad_(True)
    z = O._bn(F.conv2d(x, w, padding=k // 2), p, "bn")
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    z.backward(dz)
    # the folded conv's own gradients: dW' = dZ (x) X in NHWC order, db' = sum dZ
    dwf = torch.nn.grad.conv2d_weight(x.detach(), w.shape, dz, padding=k // 2).permute(0, 2, 3, 1)
    dbf = dz.sum(dim=(0, 2, 3))
    gw, gg, gb = _fold_backward(dwf, dbf, w.detach(), p["bn.weight"].detach(), p["bn.running_mean"],
                                p["bn.running_var"])
    for got, want in ((gw, w.grad), (gg, p["bn.weight"].grad), (gb, p["bn.bias"].grad)):
        assert (got - want).abs().max() <= 1e-10 * max(1.0, want.abs().max().item())
    # the input gradient is a forward conv of dZ on the flipped, channel-swapped folded weight (w_igrad's layout)
    scale = (p["bn.weight"] / torch.sqrt(p["bn.running_var"] + 1e-5)).detach()
    wf = (w.detach() * scale[:, None, None, None]).permute(0, 2, 3, 1)       # [Cout,KH,KW,Cin]
    wi = wf.flip(1, 2).permute(3, 1, 2, 0)                                    # [Cin,KH,KW,Cout]
    dx = F.conv2d(dz, wi.permute(0, 3, 1, 2), padding=k // 2)
    assert (dx - x.grad).abs().max() <= 1e-12 * max(1.0, x.grad.abs().max().item())


# ---- data parallelism: two gloo ranks end with the mean of their tail gradients ----
class _FakeEncoder:
    def __init__(self, rank):
        self.tail_grad_flat = torch.arange(37, dtype=torch.float32) * (rank + 1) + rank


def _dp_worker(rank, world, init_file, results):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    import sat_amd.distributed as D
    torch.set_num_threads(1)
    enc = _FakeEncoder(rank)
    D.all_reduce_tail_grads(enc)
    want = torch.arange(37, dtype=torch.float32) * 1.5 + 0.5
    none = _FakeEncoder(rank)
    none.tail_grad_flat = None
    D.all_reduce_tail_grads(none)   # before the first backward: nothing to reduce, no collective
    results[rank] = bool(torch.allclose(enc.tail_grad_flat, want))
    dist.destroy_process_group()


def test_tail_gradients_are_averaged_over_gloo_ranks():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mgr = mp.Manager()
        results = mgr.dict()
        mp.spawn(_dp_worker, args=(2, os.path.join(d, "init"), results), nprocs=2, join=True)
        assert dict(results) == {0: True, 1: True}

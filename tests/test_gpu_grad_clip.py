"""Gradient clipping by global norm on the device (sat_grad_sumsq, sat_grad_clip_finalize, sat_adam_step_scaled,
``sat_amd.Adam(max_grad_norm=...)``, ``train.py --clip-grad-norm``).

Bounds, none of them measured:
  * sum of squares: the square of an fp32 value is exact in fp64 and the device adds in fp64, so it differs from the
    host's fp64 sum by summation order only, about n * 2^-53 relative: 1e-12 holds for every n here (< 2^23);
  * norm: fp32(sqrt(total)) of two totals that differ by that much differ by at most one fp32 ulp: 2^-23 relative;
  * scale: one fp32 add and one fp32 divide on a norm within 2^-24 of the fp64 value: 2^-22 relative;
  * the clipped step against plain Adam on gradients pre-multiplied by the same fp32 scale: the same bits;
  * against torch alone (clip_grad_norm_ + torch.optim.Adam): 1e-6 relative on the norm, 1e-6 absolute per weight,
    the bound the fused Adam is already held to.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import sat_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = 4096          # fp32 elements one workgroup reads per loop trip
GRID = 8              # workgroups of the path tests: a whole-grid sweep is GRID * SWEEP elements
V, D, B, T, LF = 50, 64, 3, 5, 4


@pytest.fixture(scope="module")
def sat():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import sat_amd
    return sat_amd


# ---------------------------------------------------------------------------- 1. sum of squares on every path
@pytest.fixture(scope="module")
def buffer():
    """Seeded fp32 values with magnitudes over 1e-12 ... 1e6, on the host (read-only) and on the device."""
    rng = np.random.default_rng(5)
    n = 1024 * SWEEP + 16
    host = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 6, n)).astype(np.float32)
    host.setflags(write=False)
    return host, torch.from_numpy(host.copy()).to(DEV)


def _host_sumsq(host, off, n):
    return float(np.sum(host[off:off + n].astype(np.float64) ** 2))


LENGTHS = [1, 3, 4, 5,
           SWEEP - 1, SWEEP, SWEEP + 1,               # around one workgroup's sweep (start offset 0: no head)
           SWEEP + 2, SWEEP + 3, SWEEP + 4,           # the same behind the 3-element head of start offset 1
           GRID * SWEEP + 5, GRID * SWEEP + 3 + 5,    # above one sweep of the whole grid
           2 * SWEEP + 9]                             # most of the GRID workgroups have no share


@pytest.mark.parametrize("offset", [0, 1])
def test_sumsq_every_path(sat, buffer, offset):
    host, dev = buffer
    for n in LENGTHS:
        g = dev[offset:offset + n]
        assert g.data_ptr() % 16 == 4 * offset
        ref = _host_sumsq(host, offset, n)
        outs = []
        for _ in range(2):
            partials = torch.full((GRID,), math.nan, device=DEV, dtype=torch.float64)
            sat.ops.grad_sumsq(g, partials)
            outs.append(partials)
        got = outs[0].cpu().numpy()
        assert np.isfinite(got).all(), (n, offset, got)
        empty = max(0, GRID - -(-n // SWEEP))   # at least this many workgroups have no share
        assert (got == 0).sum() >= empty, (n, offset, got)
        err = abs(float(got.sum()) - ref) / ref
        print(f"sumsq n={n} offset={offset} rel err {err:.3e}")
        assert err <= 1e-12, (n, offset, err)
        assert torch.equal(outs[0], outs[1]), (n, offset)


@pytest.mark.parametrize("offset", [0, 1])
def test_sumsq_optimiser_grid(sat, buffer, offset):
    """The grid the optimiser uses (1024 workgroups) one sweep of the whole grid plus 5."""
    host, dev = buffer
    n = 1024 * SWEEP + 5
    g = dev[offset:offset + n]
    count = sat.ops.grad_sumsq_partials(n)
    assert count == 1024
    outs = [sat.ops.grad_sumsq(g, torch.full((count,), math.nan, device=DEV, dtype=torch.float64)) for _ in range(2)]
    ref = _host_sumsq(host, offset, n)
    err = abs(float(outs[0].cpu().numpy().sum()) - ref) / ref
    print(f"sumsq n={n} offset={offset} rel err {err:.3e}")
    assert err <= 1e-12 and torch.equal(outs[0], outs[1])


def _scale64(max_norm, norm64):
    return min(1.0, max_norm / (norm64 + 1e-6))


@pytest.mark.parametrize("ranges", [((0, SWEEP + 1), (1, 5)), ((1, GRID * SWEEP + 5), (0, 3)),
                                    ((7, 2 * SWEEP + 9), (SWEEP, SWEEP))])
def test_finalize_two_ranges(sat, buffer, ranges):
    host, dev = buffer
    counts = [sat.ops.grad_sumsq_partials(n) for _, n in ranges]
    ws = torch.full((sum(counts),), math.nan, device=DEV, dtype=torch.float64)
    at = 0
    for (off, n), c in zip(ranges, counts):
        sat.ops.grad_sumsq(dev[off:off + n], ws[at:at + c])
        at += c
    total = sum(_host_sumsq(host, off, n) for off, n in ranges)
    norm64 = math.sqrt(total)
    norm32 = float(np.float32(norm64))
    state = torch.zeros(4, device=DEV)
    for factor in (0.5, 0.999, 2.0):
        max_norm = float(np.float32(factor * norm64))
        sat.ops.grad_clip_finalize(ws, max_norm, state)
        norm, scale, bad, skipped = state.tolist()
        e_norm = abs(norm - norm32) / norm32
        want = _scale64(max_norm, norm64)
        e_scale = abs(scale - want) / want
        print(f"finalize {ranges} x{factor}: norm rel {e_norm:.3e} scale rel {e_scale:.3e}")
        assert e_norm <= 2.0 ** -23, (norm, norm32)
        assert e_scale <= 2.0 ** -22, (scale, want)
        assert bad == 0 and skipped == 0
        if factor > 1:
            assert scale == 1.0


def test_finalize_non_finite_counts(sat):
    state = torch.zeros(4, device=DEV)
    for k, value in enumerate((math.inf, math.nan), 1):
        ws = torch.tensor([1.0, value, 4.0], device=DEV, dtype=torch.float64)
        sat.ops.grad_clip_finalize(ws, 1.0, state)
        norm, scale, bad, skipped = state.tolist()
        assert not math.isfinite(norm) and scale == 0.0 and bad == 1.0 and skipped == k
    sat.ops.grad_clip_finalize(torch.tensor([9.0, 16.0], device=DEV, dtype=torch.float64), 1.0, state)
    norm, scale, bad, skipped = state.tolist()
    assert norm == 5.0 and bad == 0.0 and skipped == 2.0
    assert abs(scale - 1.0 / (5.0 + 1e-6)) <= 2.0 ** -22 * scale


# ---------------------------------------------------------------------------- 2.-5. through the optimiser
class Rig:
    """A small decoder plus one plain un-owned fp32 tensor as a second param group with its own lr and gradient."""

    def __init__(self, sat, attention, dtype, max_grad_norm, seed=3, lr=1e-3):
        self.sat, self.dtype = sat, dtype
        torch.manual_seed(seed)
        self.dec = sat.Decoder(V, D, tf=True, attention=attention).to(DEV).eval()
        gen = torch.Generator().manual_seed(seed + 1)
        self.extra = (0.1 * torch.randn(1001, generator=gen)).to(DEV).requires_grad_(True)
        self.opt = sat.Adam([{"params": list(self.dec.parameters())}, {"params": [self.extra], "lr": 0.5 * lr}],
                            lr=lr, max_grad_norm=max_grad_norm)
        self.feats = torch.rand(B, LF, D, generator=gen).bfloat16().float().to(DEV)
        self.caps = O.make_captions(B, T, V, seed + 2).to(DEV)
        self.gen = gen

    def named(self):
        return dict(self.dec.named_parameters(), extra=self.extra)

    def backward(self, step):
        """zero_grad, forward, loss, backward; the extra tensor gets a seeded gradient of the decoder's scale."""
        self.opt.zero_grad()
        caps = torch.roll(self.caps, step, 0)
        preds, alphas = self.dec(self.feats.to(self.dtype), caps)
        loss, _ = self.sat.caption_loss(preds, alphas, caps)
        loss.backward()
        self.extra.grad = (1e-2 * torch.randn(1001, generator=self.gen)).to(DEV)

    def take_grads(self, other):
        """Overwrite this rig's gradients, in place, by ``other``'s (same parameters have one)."""
        mine, theirs = self.named(), other.named()
        for n, p in mine.items():
            assert (p.grad is None) == (theirs[n].grad is None), n
            if p.grad is not None:
                p.grad.copy_(theirs[n].grad)

    def host_norm(self):
        """fp64 norm over exactly the parameters that have a .grad."""
        return math.sqrt(sum(float(p.grad.detach().double().pow(2).sum()) for p in self.named().values()
                             if p.grad is not None))

    def snapshot(self):
        out = {}
        for n, p in self.named().items():
            out[n] = p.detach().clone()
            st = self.opt.state.get(p, {})
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    out[n + "." + k] = st[k].detach().clone()
        if self.dec._flat_lp is not None:
            out["shadow"] = self.dec._flat_lp.detach().clone()
        return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a.keys() ^ b.keys()))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, (a[k].float() - b[k].float()).abs().max().item())


CASES = [(True, torch.float32), (True, torch.bfloat16), (False, torch.bfloat16)]
CASE_IDS = ["attention-fp32", "attention-bf16", "no_attention-bf16"]


@pytest.mark.parametrize("factor", [0.5, 2.0])
@pytest.mark.parametrize("attention,dtype", CASES, ids=CASE_IDS)
def test_clipped_step_equals_adam_on_scaled_gradients(sat, attention, dtype, factor):
    rig = Rig(sat, attention, dtype, max_grad_norm=1.0)
    twin = Rig(sat, attention, dtype, max_grad_norm=None)
    _assert_same(rig.snapshot(), twin.snapshot(), "initial state")
    for step in range(2):   # the second step starts from non-zero moments (and a shadow the first one wrote)
        rig.backward(step)
        twin.backward(step)
        twin.take_grads(rig)
        if not attention:   # inactive parameters: no gradient, not counted, not moved
            assert any(p.grad is None for p in rig.dec.parameters())
        norm64 = rig.host_norm()
        rig.opt.max_grad_norm = float(np.float32(factor * norm64))
        rig.opt.step()
        e_norm = abs(float(rig.opt.grad_norm) - norm64) / norm64
        scale = float(rig.opt.clip_scale)
        print(f"step {step}: norm {norm64:.6e} rel err {e_norm:.3e} scale {scale!r}")
        assert e_norm <= 2.0 ** -23
        assert rig.opt.grad_norm.dim() == 0 and rig.opt.grad_norm.device.type == "cuda"
        assert float(rig.opt.skipped_steps) == 0
        if factor > 1:
            assert scale == 1.0
        else:
            want = _scale64(rig.opt.max_grad_norm, norm64)
            assert abs(scale - want) <= 2.0 ** -22 * want and scale < 0.51
            for p in twin.named().values():   # torch's fp32 multiply on the device, in place
                if p.grad is not None:
                    p.grad.mul_(rig.opt.clip_scale)
        twin.opt.step()
        if dtype == torch.bfloat16:
            assert rig.dec._flat_lp is not None
        _assert_same(rig.snapshot(), twin.snapshot(), f"after step {step}")


def test_clipped_steps_match_torch(sat):
    rig = Rig(sat, True, torch.float32, max_grad_norm=1.0)
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in rig.named().items()}
    ropt = torch.optim.Adam([{"params": [p for n, p in ref.items() if n != "extra"]},
                             {"params": [ref["extra"]], "lr": 0.5e-3}], lr=1e-3)
    max_norm = None
    for step in range(3):
        rig.backward(step)
        if max_norm is None:
            max_norm = float(np.float32(0.5 * rig.host_norm()))
            rig.opt.max_grad_norm = max_norm
        for n, p in rig.named().items():
            ref[n].grad = None if p.grad is None else p.grad.detach().clone()
        total = torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm)
        ropt.step()
        rig.opt.step()
        e_norm = abs(float(total) - float(rig.opt.grad_norm)) / float(total)
        print(f"step {step}: torch norm {float(total):.6e} rel diff {e_norm:.3e} scale {float(rig.opt.clip_scale)!r}")
        assert e_norm <= 1e-6
        assert float(rig.opt.clip_scale) < 1.0
    worst = max((p.detach() - ref[n].detach()).abs().max().item() for n, p in rig.named().items())
    print(f"largest weight difference to torch after 3 steps {worst:.3e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("value,where", [(math.inf, "lstm.weight_ih"), (math.nan, "extra")])
def test_non_finite_gradient_skips_the_step(sat, value, where):
    rig = Rig(sat, True, torch.bfloat16, max_grad_norm=1.0)
    twin = Rig(sat, True, torch.bfloat16, max_grad_norm=None)
    for step in range(3):
        rig.backward(step)
        twin.backward(step)
        twin.take_grads(rig)
        if step == 0:
            rig.opt.max_grad_norm = float(np.float32(0.5 * rig.host_norm()))
        if step == 1:   # one bad value: nothing may move, the step is counted
            rig.named()[where].grad.view(-1)[7] = value
            before = rig.snapshot()
            rig.opt.step()
            _assert_same(rig.snapshot(), before, f"skipped step ({value})")
            assert float(rig.opt.skipped_steps) == 1 and float(rig.opt.clip_scale) == 0
            assert not math.isfinite(float(rig.opt.grad_norm))
            for p in twin.named().values():   # the host step count advances on a skipped step: so does the twin's
                if p.grad is not None:
                    twin.opt.state[p]["step"] += 1
            continue
        rig.opt.step()
        for p in twin.named().values():
            if p.grad is not None:
                p.grad.mul_(rig.opt.clip_scale)
        twin.opt.step()
        _assert_same(rig.snapshot(), twin.snapshot(), f"after step {step}")
    assert float(rig.opt.skipped_steps) == 1
    assert all(int(rig.opt.state[p]["step"]) == 3 for p in rig.named().values() if p.grad is not None)


def test_clipped_step_does_not_wait_for_the_device(sat):
    rig = Rig(sat, True, torch.bfloat16, max_grad_norm=1e-3)
    rig.backward(0)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raises = False
        except RuntimeError:
            raises = True
        if raises:
            rig.opt.step()   # the first step also creates the state and the workspace
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raises:
        pytest.skip("this torch build does not raise on a synchronising call under set_sync_debug_mode('error')")
    rig.backward(1)
    torch.cuda.set_sync_debug_mode("error")
    try:
        rig.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert 0 < float(rig.opt.clip_scale) < 1 and float(rig.opt.skipped_steps) == 0


def test_mixed_devices_refused(sat):
    a = torch.zeros(4, device=DEV, requires_grad=True)
    b = torch.zeros(4, requires_grad=True)
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    opt = sat.Adam([a, b], max_grad_norm=1.0)
    with pytest.raises(ValueError, match="one device"):
        opt.step()
    assert len(opt.state) == 0


# ---------------------------------------------------------------------------- 6. train.py end to end
def test_train_cli_clip_grad_norm(sat, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(REPO, "show-attend-and-tell_amd", "train.py"),
                          "--synthetic", "32", "--batch-size", "16", "--max-steps", "2", "--epochs", "1",
                          "--clip-grad-norm", "0.01", "--network", "vgg19", "--tf", "--ado", "--attention",
                          "--vocab", "300", "--log-interval", "1", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{") and "train_loss" in l]
    assert len(recs) == 2, out.stdout[-2000:]
    for r in recs:
        assert math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0.01, r
        assert r["skipped_steps"] == 0, r

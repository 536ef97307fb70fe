"""Adam on the HIP path (reference optimiser: train.py:71-72,100,164).

``Adam(params, lr, betas, eps)`` is a torch.optim.Optimizer (so
``torch.optim.lr_scheduler.StepLR`` drives it exactly as in the reference) whose
step runs ``sat_adam_step``: torch's single-tensor Adam arithmetic
(``exp_avg.lerp_``, ``exp_avg_sq.mul_().addcmul_()``, ``addcdiv_`` with the
bias corrections), fused, one launch per contiguous range of a decoder's flat
parameter buffer, also refreshing the decoder's bf16 weight shadow.  Params
whose grad is None are skipped and keep no state, as in torch.

``max_grad_norm=C`` clips by global norm inside the step, on the device:
``sat_grad_sumsq`` per range into fp64 partials, one ``sat_grad_clip_finalize``
(norm over every param group, ``scale = min(1, C / (norm + 1e-6))`` as
``torch.nn.utils.clip_grad_norm_``), then ``sat_adam_step_scaled`` per range,
which multiplies the gradient by the scale as it reads it (``.grad`` itself is
left unscaled).  The step issues no device-to-host copy and no synchronise;
``grad_norm``, ``clip_scale`` and ``skipped_steps`` are 0-d views of the device
state.  A non-finite norm skips the update: parameters, moments and the bf16
shadow stay as they were and ``skipped_steps`` grows by one.  The host step
counter still advances on a skipped step, so the bias corrections follow the
calls of ``step()``, not the updates that were applied.  ``None`` (the default)
is the unclipped step: the same launches as before the option existed.
"""
import math

import torch

from . import ops


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None):
        if weight_decay != 0:
            raise ValueError("sat_amd.optim.Adam: weight_decay is not used by the reference (train.py:71)")
        self.max_grad_norm = max_grad_norm   # validated before the base class looks at params
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._flat_state = {}   # id(owner flat) -> (exp_avg flat, exp_avg_sq flat)
        self._clip_state = None   # device fp32 [norm, scale, non-finite flag, skipped steps] (sat_grad_clip_finalize)
        self._clip_ws = None      # device fp64 partials of every run (sat_grad_sumsq)

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if value is not None:
            try:
                v = float(value)
            except (TypeError, ValueError):
                v = math.nan
            if not (0 < v <= torch.finfo(torch.float32).max):   # the kernels take it as fp32
                raise ValueError(f"sat_amd.optim.Adam: max_grad_norm must be a finite number > 0, got {value!r}")
            value = v
        self._max_grad_norm = value

    def _clip_view(self, i):
        return None if self._clip_state is None else self._clip_state[i]

    @property
    def clip_state(self):
        """The device state of clipping, fp32 [norm, scale, non-finite flag, skipped steps] (None before a step)."""
        return self._clip_state

    @property
    def grad_norm(self):
        """Global L2 norm of the last clipped step's gradients: a 0-d view of the device state (None before one)."""
        return self._clip_view(0)

    @property
    def clip_scale(self):
        """What the last clipped step multiplied the gradients by (0 on a skipped step): 0-d device view."""
        return self._clip_view(1)

    @property
    def skipped_steps(self):
        """How many clipped steps found a non-finite norm and changed nothing: 0-d device view."""
        return self._clip_view(3)

    def _owner(self, p):
        ref = getattr(p, "_sat_owner", None)
        owner = ref() if ref is not None else None
        if owner is None or owner._flat is None:
            return None
        if p.data_ptr() != owner._flat.data_ptr() + 4 * p._sat_offset:
            return None
        return owner

    def _state_for(self, p, owner):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)
            if owner is not None:
                key = id(owner._flat)
                if key not in self._flat_state:
                    self._flat_state[key] = (torch.zeros_like(owner._flat), torch.zeros_like(owner._flat))
                m, v = self._flat_state[key]
                o = p._sat_offset
                st["exp_avg"] = m[o:o + p.numel()].view(p.shape)
                st["exp_avg_sq"] = v[o:o + p.numel()].view(p.shape)
            else:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _collect(self, group):
        """The parameters of ``group`` that have a gradient (step counters advanced) and the contiguous ranges
        (runs) that one launch each updates."""
        items = []
        for p in group["params"]:
            if p.grad is None:
                continue
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("sat_amd.optim.Adam: fp32 contiguous parameters only")
            owner = self._owner(p)
            st = self._state_for(p, owner)
            st["step"] += 1
            items.append((p, owner, st))
        # merge runs of params that are adjacent in one flat buffer (same step count); a run also spans the
        # alignment padding between two parameter groups (< 64 floats holding no parameter: zero value,
        # gradient and moments, which the update leaves at zero), so one launch covers a whole flat buffer
        runs = []
        for p, owner, st in sorted(items, key=lambda it: (id(it[1]), it[0].data_ptr())):
            step = int(st["step"].item())
            gap = (p.data_ptr() - runs[-1]["end_ptr"]) // 4 if runs else -1
            padding_only = (runs and owner is not None and runs[-1]["owner"] is owner and 0 < gap < 64
                            and not any(runs[-1]["end_off"] <= o < p._sat_offset for o in owner._offsets.values()))
            contiguous_with_prev = (runs and owner is not None and runs[-1]["owner"] is owner
                                    and runs[-1]["step"] == step
                                    and (gap == 0 or padding_only)
                                    and runs[-1]["gend"] + 4 * gap == p.grad.data_ptr()
                                    and runs[-1]["mend"] + 4 * gap == st["exp_avg"].data_ptr())
            if contiguous_with_prev:
                r = runs[-1]
                r["n"] += gap + p.numel()
            else:
                runs.append(dict(owner=owner, step=step, p=p, st=st, n=p.numel()))
                r = runs[-1]
            r["end_ptr"] = p.data_ptr() + 4 * p.numel()
            r["end_off"] = (p._sat_offset + p.numel()) if owner is not None else 0
            r["gend"] = p.grad.data_ptr() + 4 * p.numel()
            r["mend"] = st["exp_avg"].data_ptr() + 4 * p.numel()
        return items, runs

    def _update(self, group, runs, clip_state):
        """One Adam launch per run; ``clip_state`` (device, from the finalize) selects the scaled kernel."""
        lr, (b1, b2), eps = group["lr"], group["betas"], group["eps"]
        for r in runs:
            p, st, n, owner = r["p"], r["st"], r["n"], r["owner"]
            bc1 = 1 - b1 ** r["step"]
            bc2 = 1 - b2 ** r["step"]
            off = p._sat_offset if owner is not None else 0
            lp = None
            if owner is not None and owner._flat_lp is not None:
                lp = owner._flat_lp[off:off + n]
                owner._lp_versions = None if lp is None else owner._lp_versions
            gv = self._run_grad(r)
            if owner is not None:
                pv = owner._flat[off:off + n]
                m, v = self._flat_state[id(owner._flat)]
                mv, vv = m[off:off + n], v[off:off + n]
            else:
                pv, mv, vv = p.view(-1), st["exp_avg"].view(-1), st["exp_avg_sq"].view(-1)
                # the kernel writes through the pointer: tell whoever keys on the parameter's version (the
                # encoder's plan refresh of a fine-tuned tail) that it changed
                torch.autograd.graph.increment_version(p)
            if clip_state is None:
                ops.adam_step_(pv, gv, mv, vv, lp, b1, b2, eps, lr / bc1, math.sqrt(bc2))
            else:
                ops.adam_step_scaled_(pv, gv, mv, vv, lp, b1, b2, eps, lr / bc1, math.sqrt(bc2), clip_state)

    def _refresh(self, items):
        refreshed = set()
        for p, owner, st in items:
            if owner is not None and owner._flat_lp is not None:
                owner._lp_versions = tuple(q._version for q in owner.parameters())
                if id(owner) not in refreshed:   # the transposed copies follow the updated shadow
                    refreshed.add(id(owner))
                    owner.refresh_transposed()

    @staticmethod
    def _run_grad(r):
        """The gradient range a run's update reads."""
        if r["owner"] is not None:
            off = r["p"]._sat_offset
            return r["owner"]._grad_flat[off:off + r["n"]]
        return r["p"].grad.view(-1)

    def _clip(self, collected):
        """Partials of every run, then one finalize: leaves norm, scale and the non-finite flag in ``_clip_state``."""
        runs = [r for _, runs in collected for r in runs]
        if not runs:
            return False
        device = runs[0]["p"].device
        counts = [ops.grad_sumsq_partials(r["n"]) for r in runs]
        if self._clip_state is None or self._clip_state.device != device:
            self._clip_state = torch.zeros(4, device=device, dtype=torch.float32)
        if self._clip_ws is None or self._clip_ws.numel() < sum(counts) or self._clip_ws.device != device:
            self._clip_ws = torch.empty(sum(counts), device=device, dtype=torch.float64)
        at = 0
        for r, c in zip(runs, counts):
            ops.grad_sumsq(self._run_grad(r), self._clip_ws[at:at + c])
            at += c
        ops.grad_clip_finalize(self._clip_ws[:at], self.max_grad_norm, self._clip_state)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is None:
            for group in self.param_groups:
                items, runs = self._collect(group)
                self._update(group, runs, None)
                self._refresh(items)
            return loss
        devices = {p.device for group in self.param_groups for p in group["params"] if p.grad is not None}
        if len(devices) > 1:
            raise ValueError("sat_amd.optim.Adam: max_grad_norm needs every parameter on one device, got "
                             f"{sorted(map(str, devices))}")
        collected = [self._collect(group) for group in self.param_groups]
        if self._clip(collected):
            for group, (items, runs) in zip(self.param_groups, collected):
                self._update(group, runs, self._clip_state)
                self._refresh(items)
        return loss

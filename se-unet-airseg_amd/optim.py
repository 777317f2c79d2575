"""Fused AdamW for the MI355X hot path.

Drop-in for the reference's ``torch.optim.AdamW(model.parameters(), lr=0.0001)`` (train.py:188,386,569) and its
``optimizer.step()`` (train.py:247,439,603): same constructor arguments, ``param_groups`` / ``state`` layout (so
``torch.optim.lr_scheduler.MultiStepLR`` at train.py:189-191 and ``state_dict()`` keep working), but one native
multi-tensor launch sequence per step (``seunet_adamw_step``, csrc/optim.hip) instead of PyTorch's per-op foreach
kernels.  There is no CPU path: parameters must be contiguous float32 CUDA tensors.

Overflow gate (fp16 storage): ``AdamW(..., overflow_gate=model)`` or ``opt.bind_overflow_gate(model)`` makes the step behind a
backward pass whose scaled gradients overflowed a true no-op -- parameters, ``exp_avg`` and ``exp_avg_sq`` keep their bits and
later bias corrections count applied steps only.  The gate is ``model.overflow_pending``, a device int32 flag that ``SE_UNet``'s
backward sets (and never clears) on an overflow; it is looked up at ``step()`` time, read by the kernels in stream order with
no host synchronisation (``seunet_adamw_step_gated``), and cleared by ``step()`` once consumed -- so with gradient accumulation
one overflowing backward skips the step that follows.  ``state['step']`` still counts every ``step()`` call; the per-tensor
device count ``state['skipped']`` (a whole number held in an f32, so that ``load_state_dict`` leaves it as it is) is what the
kernels subtract.  A gate that does not exist yet or never will (no forward so far; bf16 / fp32 storage) runs the ungated code.
"""
import ctypes as C
from typing import Iterable, Tuple

import torch

from . import _lib


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (decoupled weight decay, bias correction, no amsgrad) on the HIP library."""

    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, *, maximize: bool = False, overflow_gate=None):
        if amsgrad:
            raise ValueError("seunet AdamW: amsgrad is not implemented (the reference never enables it)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=maximize))
        self._overflow_gate = overflow_gate

    def bind_overflow_gate(self, gate) -> None:
        """``gate``: an ``SE_UNet`` (its ``overflow_pending`` flag is looked up at every ``step()``), a device int32 tensor of one
        element (non-zero = skip the next step; ``step()`` clears it), or None for the ungated step."""
        self._overflow_gate = gate

    def _skip_flag(self):
        gate = self._overflow_gate
        flag = gate if gate is None or torch.is_tensor(gate) else getattr(gate, "overflow_pending", None)
        if flag is not None and not (flag.is_cuda and flag.dtype == torch.int32 and flag.numel() == 1):
            raise RuntimeError("seunet AdamW: the overflow gate must be one int32 element on the GPU")
        return flag

    def _init_group_state(self, group):
        """exp_avg / exp_avg_sq of a group live in one flat buffer each (views per parameter)."""
        todo = [p for p in group["params"] if p.grad is not None and len(self.state[p]) == 0]
        if not todo:
            return
        dev = todo[0].device
        total = sum(p.numel() for p in todo)
        flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        for p in todo:
            n = p.numel()
            st = self.state[p]
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = flat_m[off:off + n].view_as(p)
            st["exp_avg_sq"] = flat_v[off:off + n].view_as(p)
            off += n

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        flag = self._skip_flag()
        for group in self.param_groups:
            self._init_group_state(group)
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError("seunet AdamW: parameters must be contiguous float32 CUDA tensors (no CPU path)")
                if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                    raise RuntimeError("seunet AdamW: gradients must be dense float32 tensors on the parameter's device")
                st = self.state[p]
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append((p, g if g.is_contiguous() else g.contiguous(), st))
            beta1, beta2 = group["betas"]
            if flag is not None and by_step:
                self._gated_group_step(lib, group, by_step, flag)
                continue
            for step, items in by_step.items():
                n = len(items)
                pa, ga, ma, va = ((C.c_void_p * n)() for _ in range(4))
                cnt = (C.c_longlong * n)()
                for i, (p, g, st) in enumerate(items):
                    pa[i], ga[i] = p.data_ptr(), g.data_ptr()
                    ma[i], va[i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    cnt[i] = p.numel()
                with torch.cuda.device(items[0][0].device):
                    _lib.check(lib.seunet_adamw_step(pa, ga, ma, va, cnt, n, float(group["lr"]), float(beta1), float(beta2),
                                                     float(group["eps"]), float(group["weight_decay"]), step,
                                                     int(bool(group["maximize"])), _lib.stream_ptr()), "adamw_step")
        if flag is not None:
            flag.zero_()        # consumed (stream-ordered behind the kernels that read it)
        return loss

    def _gated_group_step(self, lib, group, by_step, flag):
        """All tensors of the group in one call: each carries its own step and skipped count, the kernels decide."""
        items = [(step, *it) for step, its in by_step.items() for it in its]
        n = len(items)
        dev = items[0][1].device
        if flag.device != dev:
            raise RuntimeError(f"seunet AdamW: the overflow gate is on {flag.device} but the parameters are on {dev}")
        new = [st for _, _, _, st in items if "skipped" not in st]
        if new:
            flat = torch.zeros(len(new), dtype=torch.float32, device=dev)
            for i, st in enumerate(new):
                st["skipped"] = flat[i]
        pa, ga, ma, va, sa = ((C.c_void_p * n)() for _ in range(5))
        cnt, steps = (C.c_longlong * n)(), (C.c_int * n)()
        for i, (step, p, g, st) in enumerate(items):
            sk = st["skipped"]
            if not (sk.is_cuda and sk.dtype == torch.float32 and sk.numel() == 1 and sk.device == dev):
                raise RuntimeError("seunet AdamW: state['skipped'] must be one float32 element on the parameter's device")
            pa[i], ga[i] = p.data_ptr(), g.data_ptr()
            ma[i], va[i], sa[i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), sk.data_ptr()
            cnt[i], steps[i] = p.numel(), step
        beta1, beta2 = group["betas"]
        with torch.cuda.device(dev):
            table = torch.empty(2 * n, dtype=torch.float32, device=dev)     # step_size, 1/sqrt(bc2) per tensor: written by the prepare kernel
            _lib.check(lib.seunet_adamw_step_gated(pa, ga, ma, va, cnt, steps, sa, n, float(group["lr"]), float(beta1), float(beta2),
                                                   float(group["eps"]), float(group["weight_decay"]), int(bool(group["maximize"])),
                                                   flag.data_ptr(), table.data_ptr(), _lib.stream_ptr()), "adamw_step_gated")

"""``torch.optim.Adam`` (what the reference trains with, ``/root/reference/src/train.py:469``) as ONE kernel launch per step
(``csrc/optim.hip``) plus one ``_foreach_add_`` on the step counters.

At dataset scale the parameter set is ~20 small tensors; torch's fused multi-tensor Adam in capturable mode spends ~40 us on
them -- a tenth of a hipGraph-replayed Cora step.  Same arithmetic (non-amsgrad, L2 ``weight_decay``, bias corrections from a
per-parameter step counter kept on the device, so the optimizer is capturable by construction); fp32 and bf16 device
parameters (bf16: moments in bf16 as torch keeps them, fp32 arithmetic); anything else falls back to ``torch.optim.Adam``'s functional form.

``master_weights=True`` is mixed-precision training: a bf16 parameter keeps an fp32 master weight and fp32
moments in the optimizer's state, the update runs on those (``adam_master_kernel``, the same launch shape), and the bf16 parameter
is rewritten as the one rounding of its master.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from itertools import chain
from typing import Iterable

import torch

from . import _lib
from ._lib import check, stream_of, on_device

_MASTER_KEYS = ("master", "exp_avg", "exp_avg_sq")          # fp32 whatever the parameter's dtype (see load_state_dict)


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` -- the form the reference uses -- on fp32 / bf16 device
    parameters.  NOT covered, and refused rather than ignored: ``amsgrad``, ``maximize``, a tensor ``lr``.

    ``master_weights`` (a group option, default False): every bfloat16 parameter of the group is trained through an fp32 master
    weight.  Its state is ``step``, ``master`` (fp32, created as ``p.detach().float()`` at the parameter's first step), ``exp_avg``
    and ``exp_avg_sq`` (fp32); after every step ``p`` equals ``master.to(torch.bfloat16)`` bit for bit.  With bf16 moments and a bf16
    parameter (the default form) an update below half a bf16 spacing -- ``lr`` 1e-3 against 2^-8 near 1.0 -- is rounded away at every
    step; the master accumulates it.  fp32 parameters of such a group, and every group without the option, behave as before.
    ``load_state_dict`` keeps the three fp32 state tensors fp32 (the stock method casts them to the parameter's dtype);
    :meth:`sync_masters` re-reads the masters after the parameters were overwritten from outside; :meth:`master_state_dict` is the
    model's ``state_dict`` in full precision."""

    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, maximize: bool = False, master_weights: bool = False):
        if amsgrad or maximize:
            raise NotImplementedError("FusedAdam covers plain Adam only (no amsgrad / maximize): use torch.optim.Adam")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("FusedAdam takes a float learning rate (the kernel receives it by value)")
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("FusedAdam: invalid hyper-parameter")
        # `capturable` is what allset_amd.graphs.GraphedTrainStep checks: this optimizer keeps its step counters on the device
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=True,
                                      master_weights=bool(master_weights)))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:                      # (a state dict saved before the option existed)
            group.setdefault("master_weights", False)

    @staticmethod
    def _takes_master(group, p) -> bool:
        return bool(group.get("master_weights", False)) and p.dtype == torch.bfloat16

    def _state(self, p, master: bool = False):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            if master:
                st["master"] = p.detach().float()
                st["exp_avg"] = torch.zeros_like(st["master"], memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(st["master"], memory_format=torch.preserve_format)
            else:
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step = st["step"]
        # a state loaded from a non-capturable torch.optim.Adam checkpoint carries a Python number or a CPU tensor here; the kernel
        # takes the counter's DEVICE address
        if not isinstance(step, torch.Tensor) or step.device != p.device or step.dtype != torch.float32 or step.dim() != 0:
            st["step"] = torch.as_tensor(float(step), dtype=torch.float32).to(p.device).reshape(())
        if master and "master" not in st:                    # a state of the bf16-moment form: continue from it in fp32
            st["master"] = p.detach().float()
        for k in (_MASTER_KEYS if master else _MASTER_KEYS[1:]):
            if st[k].device != p.device or (master and st[k].dtype != torch.float32):
                st[k] = st[k].to(device=p.device, dtype=torch.float32 if master else st[k].dtype)
        return st

    @staticmethod
    def _fused(p) -> bool:
        """Device, contiguous, gradient of the parameter's own type: the kernels' operands."""
        return (p.is_cuda and p.dtype in (torch.float32, torch.bfloat16) and p.is_contiguous() and p.grad.is_contiguous()
                and p.grad.dtype == p.dtype and not p.grad.is_sparse)

    def step_counters(self):
        """The device step counters ``step()`` will advance: one per parameter that has a gradient and takes a fused kernel.  A
        caller that advances them itself (``graphs.GraphedTrainStep``: in the launch that reduces the gradients) then calls
        ``step(counters_advanced=True)``."""
        out = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None and self._fused(p):
                    out.append(self._state(p, self._takes_master(group, p))["step"])
        return out

    def sync_masters(self):
        """Re-read every master weight from its parameter, in place (a captured graph holds the masters' addresses): after
        ``model.reset_parameters()`` or ``model.load_state_dict()`` on a live optimizer, whose masters would otherwise overwrite the
        new parameters at the next step.  Moments and step counters are left as they are."""
        with torch.no_grad():
            for group in self.param_groups:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and "master" in st:
                        st["master"].copy_(p.detach())

    def master_state_dict(self, model: torch.nn.Module):
        """``model.state_dict()`` with each bf16 parameter this optimizer trains through a master replaced by (a copy of) that fp32
        master -- the checkpoint to keep: the bf16 parameters are its rounding.  A parameter that has not been stepped yet has no
        master: its own value, as fp32."""
        mine = {p: group for group in self.param_groups for p in group["params"]}
        out = OrderedDict(model.state_dict())
        for name, p in model.named_parameters():
            if name in out and p in mine and self._takes_master(mine[p], p):
                st = self.state.get(p)
                out[name] = (st["master"].detach().clone() if st and "master" in st else p.detach().float())
        return out

    def load_state_dict(self, state_dict):
        """``torch.optim.Optimizer.load_state_dict`` casts every floating state tensor except ``step`` to the PARAMETER's dtype: an fp32
        master or moment of a bf16 parameter would come back as bfloat16, its low bits gone.  Those three are taken from
        ``state_dict`` again as they were saved (fp32, moved to the parameter's device)."""
        super().load_state_dict(state_dict)
        saved = state_dict["param_groups"]
        id_map = dict(zip(chain.from_iterable(g["params"] for g in saved),
                          chain.from_iterable(g["params"] for g in self.param_groups)))
        for pid, sst in state_dict["state"].items():
            p = id_map.get(pid)
            if p is None or not isinstance(sst, dict) or "master" not in sst:
                continue
            for k in _MASTER_KEYS:
                self.state[p][k] = sst[k].detach().to(device=p.device, dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None, counters_advanced: bool = False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        cap = int(lib.allset_adam_max_tensors())
        for group in self.param_groups:
            b1, b2 = group["betas"]
            live = [p for p in group["params"] if p.grad is not None]
            fast = [p for p in live if self._fused(p)]
            slow = [p for p in live if all(p is not q for q in fast)]
            slow_master = [p for p in slow if self._takes_master(group, p)]
            slow = [p for p in slow if all(p is not q for q in slow_master)]
            import importlib
            adam = importlib.import_module("torch.optim.adam").adam
            if slow:     # anything else: torch's own functional Adam on the same state layout
                sts = [self._state(p) for p in slow]
                adam(slow, [p.grad for p in slow], [s["exp_avg"] for s in sts], [s["exp_avg_sq"] for s in sts], [],
                     [s["step"] for s in sts], amsgrad=False, beta1=b1, beta2=b2, lr=group["lr"],
                     weight_decay=group["weight_decay"], eps=group["eps"], maximize=False,
                     capturable=all(p.is_cuda for p in slow),
                     foreach=None, fused=None)
            if slow_master:     # (a CPU or non-contiguous bf16 parameter: the same on its fp32 master, then the one rounding)
                sts = [self._state(p, True) for p in slow_master]
                adam([s["master"] for s in sts], [p.grad.float() for p in slow_master], [s["exp_avg"] for s in sts],
                     [s["exp_avg_sq"] for s in sts], [], [s["step"] for s in sts], amsgrad=False, beta1=b1, beta2=b2, lr=group["lr"],
                     weight_decay=group["weight_decay"], eps=group["eps"], maximize=False,
                     capturable=all(p.is_cuda for p in slow_master), foreach=None, fused=None)
                for p, s in zip(slow_master, sts):
                    p.copy_(s["master"])
            if not fast:
                continue
            sts = [self._state(p, self._takes_master(group, p)) for p in fast]
            if not counters_advanced:
                torch._foreach_add_([s["step"] for s in sts], 1.0)
            by_dev = {}
            for p, s in zip(fast, sts):
                by_dev.setdefault((p.device, p.dtype, self._takes_master(group, p)), []).append((p, s))
            for (dev, dt, master), items in by_dev.items():
                for k0 in range(0, len(items), cap):
                    part = items[k0:k0 + cap]
                    n = len(part)
                    arr = lambda vals: (ctypes.c_void_p * n)(*vals)
                    tail = ((ctypes.c_int64 * n)(*[p.numel() for p, _ in part]), n, float(group["lr"]), float(b1), float(b2),
                            float(group["eps"]), float(group["weight_decay"]), stream_of(dev))
                    with on_device(dev):
                        if master:
                            check(lib.allset_adam_master_step(arr([p.data_ptr() for p, _ in part]), arr([p.grad.data_ptr() for p, _ in part]),
                                                              arr([s["master"].data_ptr() for _, s in part]),
                                                              arr([s["exp_avg"].data_ptr() for _, s in part]),
                                                              arr([s["exp_avg_sq"].data_ptr() for _, s in part]),
                                                              arr([s["step"].data_ptr() for _, s in part]), *tail), "allset_adam_master_step")
                        else:
                            check(lib.allset_adam_step_dtype(1 if dt == torch.bfloat16 else 0, arr([p.data_ptr() for p, _ in part]),
                                                             arr([p.grad.data_ptr() for p, _ in part]),
                                                             arr([s["exp_avg"].data_ptr() for _, s in part]),
                                                             arr([s["exp_avg_sq"].data_ptr() for _, s in part]),
                                                             arr([s["step"].data_ptr() for _, s in part]), *tail), "allset_adam_step_dtype")
        return loss

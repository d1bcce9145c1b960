"""Shared machinery of the nn.Module front ends: parameter views, the autograd bridge to the
HIP engine and the flat parameter/gradient store used by the fused trainer."""
from __future__ import annotations

import os
from typing import Dict, List

import torch
import torch.nn as nn

from . import _lib as L
from .engine import Engine, NetGraph

DEFAULT_PRECISION = os.environ.get("MANTLE_PRECISION", "fp32")


class _NetFunction(torch.autograd.Function):
    """y = engine.forward(x); backward runs the HIP backward and hands parameter gradients to autograd (and the input's, for
    a graph built with input_grad)."""

    @staticmethod
    def forward(ctx, mod, x, *plist):
        eng = mod.engine()
        params = mod._param_dict(plist)
        out = eng.forward(x, params, getattr(mod, "_chan_scale", None), drop=mod._drop_next)
        mod._fwd_version += 1
        ctx.mod, ctx.params, ctx.version = mod, params, mod._fwd_version
        ctx.dtypes = [p.dtype for p in plist]
        return out

    @staticmethod
    def backward(ctx, gout):
        mod = ctx.mod
        if ctx.version != mod._fwd_version:
            raise RuntimeError("backward() through a forward pass whose device activations were overwritten by a later "
                               "forward of the same module (one in-flight forward per module)")
        names = mod._pnames
        sizes = [ctx.params[n].numel() for n in names]
        offs, off = [], 0
        for s in sizes:                          # 16-byte aligned slices (a complex view needs an even offset)
            offs.append(off)
            off = (off + s + 3) // 4 * 4
        flat = torch.zeros(off, dtype=torch.float32, device=gout.device)
        grads = {n: flat[o:o + s].view(ctx.params[n].shape) for n, o, s in zip(names, offs, sizes)}
        eng = mod.engine()
        eng.backward(gout, ctx.params, grads)
        # (a complex parameter's gradient is the interleaved (d/dRe, d/dIm) pair the engine accumulated)
        outs = [torch.view_as_complex(grads[n]).to(dt) if dt.is_complex else grads[n] if dt == torch.float32 else grads[n].to(dt)
                for n, dt in zip(names, ctx.dtypes)]
        dx = eng.input_grad() if (mod._graph.input_grad and ctx.needs_input_grad[1]) else None
        return (None, dx, *outs)


class HipNetMixin:
    """Mixed into nn.Module subclasses whose forward is one NetGraph on the HIP engine."""

    def _init_hipnet(self, graph: NetGraph, precision: str = None):
        self._graph = graph
        self._precision = precision or getattr(self, "_precision", None) or DEFAULT_PRECISION   # (keeps an earlier set_precision)
        self._engines: Dict[str, Engine] = {}
        self._fwd_version = 0
        self._drop_seed = getattr(self, "_drop_seed", None)
        self._drop_step = getattr(self, "_drop_step", 0)         # the step of a restored run (set_dropout_state), else 0
        self._pnames: List[str] = []

    @property
    def precision(self):
        return self._precision

    def set_precision(self, precision: str):
        """'fp32' (parity gate: f32 storage and arithmetic), 'bf16' (bf16 storage, f32 accumulate), 'mixed' (f16 tensors in
        the forward pass, bf16 gradient tensors: what the momentum residual needs, engine.py)."""
        if precision not in ("fp32", "bf16", "mixed"):
            raise ValueError("precision must be 'fp32', 'bf16' or 'mixed'")
        self._precision = precision
        return self

    def engine(self) -> Engine:
        e = self._engines.get(self._precision)
        if e is None:
            e = self._engines[self._precision] = Engine(self._graph, self._precision)
            self.seed_engine(e)
        return e

    def seed_engine(self, e: Engine):
        """This module's dropout seed, and a restored step (set_dropout_state), for an engine created after they were set.
        The step is the one that was restored, NOT the count the module's other engines have reached since: engines count
        their own training-mode forwards (a new engine started at 0 before there was a restored step, and still does
        without one), so an engine that is created after further training steps and must continue another engine's count
        has to be given `set_dropout_step(other.dropout_step())` by its owner."""
        e.set_dropout_seed(torch.initial_seed() if self._drop_seed is None else self._drop_seed)
        if self._drop_step:
            e.set_dropout_step(self._drop_step)

    def set_dropout_seed(self, seed: int):
        """Seed of the dropout masks (64 bits) for every engine of this module, present and future; the step counter
        restarts at 0.  The mask of a training-mode forward is a pure function of (seed, step, layer, element)."""
        self._drop_seed = int(seed)
        self._drop_step = 0
        for e in self._engines.values():
            e.set_dropout_seed(self._drop_seed)
        return self

    def dropout_seed(self) -> int:
        """The 64-bit seed the engines draw their masks from."""
        return int(torch.initial_seed() if self._drop_seed is None else self._drop_seed) & 0xFFFFFFFFFFFFFFFF

    def set_dropout_state(self, seed: int, step: int):
        """Seed and step counter together (a restored run): written into every engine that exists, in place where its
        device state is allocated, kept pending where it is not, and given to every engine created later."""
        self.set_dropout_seed(seed)
        self._drop_step = int(step) & 0xFFFFFFFF
        for e in self._engines.values():
            e.set_dropout_step(self._drop_step)
        return self

    def _named_hip_params(self):
        return list(self.named_parameters())

    def _param_dict(self, plist):
        out = {}
        for n, p in zip(self._pnames, plist):
            d = p.detach()
            if d.is_complex():               # the engine reads a complex parameter as interleaved (re, im) f32: [..., 2]
                d = torch.view_as_real(d.to(torch.complex64).contiguous())
            elif d.dtype != torch.float32:
                d = d.float()
            out[n] = d.contiguous()
        return out

    def _run_graph(self, x: torch.Tensor) -> torch.Tensor:
        L.require_cuda(x, "input")
        named = self._named_hip_params()
        self._pnames = [n for n, _ in named]
        for n, p in named:
            L.require_cuda(p, f"parameter {n}")
        # dropout follows module.training, as nn.Dropout does, except under torch.no_grad(): a forward that cannot be trained
        # through (validation, rollout) is the deterministic network
        self._drop_next = bool(self.training) and torch.is_grad_enabled()
        return _NetFunction.apply(self, x, *[p for _, p in named])


class FlatParams:
    """One flat f32 device buffer for all parameters and one for their gradients; the module's
    nn.Parameters become views, so reference-style code (state_dict, torch optimizers) keeps
    working while the fused Adam kernel and the single RCCL all-reduce see flat memory.

    A complex parameter (the spectral layers' complex64 weights) takes 2 numel f32 slots, interleaved (re, im): p.data and
    p.grad are torch.view_as_complex views of the flat buffers (slices start on multiples of 4 floats, so the views are
    aligned), views() hands the engine the real [..., 2] view, and Adam on the interleaved floats is what torch.optim.Adam
    does to a complex tensor."""

    def __init__(self, module: nn.Module, device):
        named = [(n, p) for n, p in module.named_parameters()]
        self.names = [n for n, _ in named]
        self.complex = [p.is_complex() for _, p in named]
        self.shapes = [tuple(p.shape) + ((2,) if p.is_complex() else ()) for _, p in named]      # as f32 views
        self.offsets = []
        total = 0
        for _, p in named:
            total = (total + 3) // 4 * 4      # 16-byte aligned slices
            self.offsets.append(total)
            total += p.numel() * (2 if p.is_complex() else 1)
        total = (total + 3) // 4 * 4
        self.numel = total
        self.param = torch.zeros(total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(total, dtype=torch.float32, device=device)
        self.module = module
        with torch.no_grad():
            for (n, p), off, shp, cplx in zip(named, self.offsets, self.shapes, self.complex):
                size = int(torch.Size(shp).numel())
                view = self.param[off:off + size].view(shp)
                gview = self.grad[off:off + size].view(shp)
                if cplx:
                    view.copy_(torch.view_as_real(p.detach().to(device=device, dtype=torch.complex64).contiguous()))
                    view, gview = torch.view_as_complex(view), torch.view_as_complex(gview)
                else:
                    view.copy_(p.detach().to(device=device, dtype=torch.float32))
                p.data = view
                p.grad = gview

        self._views = {}

    def views(self, flat):
        """name -> view of `flat` (cached per buffer)."""
        key = flat.data_ptr()
        v = self._views.get(key)
        if v is None:
            v = self._views[key] = {n: flat[off:off + int(torch.Size(s).numel())].view(s)
                                    for n, off, s in zip(self.names, self.offsets, self.shapes)}
        return v

    def bound(self) -> bool:
        """True while the module's parameters are still views of the flat buffer."""
        p = next(self.module.parameters())
        return p.data_ptr() == self.param.data_ptr() + 4 * self.offsets[0]

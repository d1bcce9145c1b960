"""BoundaryLearnedConvolution2D — the reference's "learned padding" layer (pytorch_networks_convae.py:802-1065; SURVEY.md
§8(f) row N4) on the HIP path: nine bias-free VALID convolutions (one on the whole input, eight on the border strips of
width k + 1 / k) framed together, plus one shared bias.

The main bank runs on the library's conv kernels (`mc_conv2d`, `mc_conv2d_wgrad*`) as a zero-padded 'same' convolution
straight into the output (its interior is the valid result); the frame of the eight border banks -- forward, filter
gradient and input gradient -- is one `mc_learned_frame_*` launch per direction that reads the input / the output
gradient in place.  As in the reference, the strip cut from the LAST rows lands in the FIRST output rows and vice versa
(:1057-1060).  Only bc_x = bc_y = 1 (output size = input size) is implemented here; the engine's learned node takes any bc.
"""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib as L
from .engine import BANKS, learned_regions
from .symmetric_layers_torch import SymmetricConv2d

_DT = {"fp32": (L.MC_F32, torch.float32), "bf16": (L.MC_BF16, torch.bfloat16)}


class _Plan:
    def __init__(self, N, H, W, c_i, c_o, k, sym_h, precision, device):
        self.key = (N, H, W, precision, str(device))
        self.N, self.H, self.W, self.c_i, self.c_o, self.k = N, H, W, c_i, c_o, k
        self.mc, self.td = _DT[precision]
        self.f = learned_regions(H, W, k)[0]                         # (fy = fx for bc = 1)
        self.ld = L.LearnedDesc(N, H, W, c_i, c_o, k, 1, 1, self.mc, sym_h)
        if L.call("mc_learned_validate", C.byref(self.ld)) != 0:
            raise ValueError("input too small for the learned-padding strips")
        dev, u8 = device, dict(dtype=torch.uint8, device=device)

        def cb8(c, h, w):
            return torch.empty((N, (c + 7) // 8, h, w, 8), dtype=self.td, device=dev)

        self.mh, self.mw = H - k + 1, W - k + 1
        # forward: 'same' convolution with zero padding f; gradients: the valid convolution (output mh x mw) and its adjoint
        self.fdesc = L.ConvDesc(N, H, W, c_i, 0, c_o, k, self.f, L.PAD_MODES["zeros"], self.mc, sym_h, 0, 0)
        self.desc = L.ConvDesc(N, H, W, c_i, 0, c_o, k, 0, L.PAD_MODES["zeros"], self.mc, sym_h, 0, 0)
        self.ddesc = L.ConvDesc(N, self.mh, self.mw, c_o, 0, c_i, k, k - 1, 0, self.mc, 0, 0, 0)
        if min(L.call("mc_conv_tiles", C.byref(d)) for d in (self.fdesc, self.desc, self.ddesc)) <= 0:
            raise L.MantleHipError("unsupported convolution configuration in BoundaryLearnedConvolution2D")
        self.bank = torch.empty(L.call("mc_packed_weight_bytes", C.byref(self.fdesc), 0), **u8)
        self.dbank = torch.empty(L.call("mc_packed_weight_bytes", C.byref(self.desc), 1), **u8)
        self.wpart = torch.empty(L.call("mc_wgrad_partial_bytes", C.byref(self.desc)), **u8)
        self.lbank = torch.empty(L.call("mc_learned_bank_bytes", C.byref(self.ld), 0), **u8)
        self.ldbank = torch.empty(L.call("mc_learned_bank_bytes", C.byref(self.ld), 1), **u8)
        self.lws = torch.empty(L.call("mc_learned_wgrad_workspace_bytes", C.byref(self.ld)), **u8)
        self.X, self.Y = cb8(c_i, H, W), cb8(c_o, H, W)
        self.dY, self.dR = cb8(c_o, H, W), cb8(c_o, self.mh, self.mw)
        self.dX = cb8(c_i, H, W)


class _LearnedConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, bias, *weights):
        L.require_cuda(x, "input")
        x = x.float().contiguous()
        N, Ci, H, W = x.shape
        p = mod._plan(N, H, W, x.device)
        st = L.stream()
        ws = {n: w.detach().float().contiguous() for n, w in zip(BANKS, weights)}
        b = bias.detach().float().reshape(-1).contiguous()
        L.call("mc_pack_nchw", L.ptr(x), N, p.c_i, Ci, H, W, 0, 0, None, p.mc, L.ptr(p.X), st)
        # the main bank's forward and input-gradient banks in one launch, the eight border banks (both directions) in another
        L.call("mc_pack_weights_batched", (L.ConvDesc * 2)(p.fdesc, p.desc), (C.c_void_p * 2)(L.ptr(ws["conv"]), L.ptr(ws["conv"])),
               (C.c_int32 * 2)(0, 1), (C.c_void_p * 2)(L.ptr(p.bank), L.ptr(p.dbank)), 2, st)
        L.call("mc_learned_pack_banks_batched", C.byref(p.ld), (C.c_void_p * 8)(*[L.ptr(ws[n]) for n in L.LEARNED_FRAME_BANKS]),
               (C.c_void_p * 1)(L.ptr(p.lbank)), (C.c_void_p * 1)(L.ptr(p.ldbank)), 1, st)
        L.call("mc_conv2d", C.byref(p.fdesc), L.ptr(p.X), None, L.ptr(p.bank), L.ptr(b), L.ptr(p.Y), None, None, st)
        L.call("mc_learned_frame_fwd", C.byref(p.ld), L.ptr(p.X), L.ptr(p.lbank), L.ptr(b), L.ptr(p.Y), st)
        out = torch.empty((N, p.c_o, H, W), dtype=torch.float32, device=x.device)
        L.call("mc_unpack_nchw", L.ptr(p.Y), N, p.c_o, H, W, 0, None, p.mc, L.ptr(out), st)
        mod._version += 1
        ctx.mod, ctx.ws, ctx.version, ctx.plan = mod, ws, mod._version, p
        ctx.wdtypes = [w.dtype for w in weights]
        ctx.bshape, ctx.bdtype = tuple(bias.shape), bias.dtype
        return out

    @staticmethod
    def backward(ctx, gout):
        mod, p, ws = ctx.mod, ctx.plan, ctx.ws
        if ctx.version != mod._version:
            raise RuntimeError("backward() through a forward pass whose device activations were overwritten by a later "
                               "forward of the same module (one in-flight forward per module)")
        N, H, W, f, st = p.N, p.H, p.W, p.f, L.stream()
        gout = gout.float().contiguous()
        dev = gout.device
        L.call("mc_pack_nchw", L.ptr(gout), N, p.c_o, p.c_o, H, W, 0, 0, None, p.mc, L.ptr(p.dY), st)
        # the main bank only sees the interior of dY: its frame belongs to the eight border banks
        L.call("mc_rect_copy", L.ptr(p.dY), H, W, f, f, L.ptr(p.dR), p.mh, p.mw, 0, 0, p.mh, p.mw, N, p.c_o, 0, p.mc, st)
        dws = {n: torch.zeros_like(ws[n]) for n in BANKS}
        db = torch.zeros(p.c_o, dtype=torch.float32, device=dev)
        L.call("mc_conv2d_wgrad", C.byref(p.desc), L.ptr(p.X), None, L.ptr(p.dR), L.ptr(p.wpart), st)
        L.call("mc_conv2d_wgrad_finalize", C.byref(p.desc), L.ptr(p.wpart), L.ptr(dws["conv"]), L.ptr(db), st)
        L.call("mc_learned_frame_wgrad", C.byref(p.ld), L.ptr(p.X), L.ptr(p.dY), L.ptr(p.lws),
               (C.c_void_p * 8)(*[L.ptr(dws[n]) for n in L.LEARNED_FRAME_BANKS]), L.ptr(db), st)
        L.call("mc_conv2d", C.byref(p.ddesc), L.ptr(p.dR), None, L.ptr(p.dbank), None, L.ptr(p.dX), None, None, st)
        L.call("mc_learned_frame_dgrad", C.byref(p.ld), L.ptr(p.dY), L.ptr(p.ldbank), L.ptr(p.dX), st)
        dx = torch.empty((N, p.c_i, H, W), dtype=torch.float32, device=dev)
        L.call("mc_unpack_nchw", L.ptr(p.dX), N, p.c_i, H, W, 0, None, p.mc, L.ptr(dx), st)
        gws = [dws[n] if dt == torch.float32 else dws[n].to(dt) for n, dt in zip(BANKS, ctx.wdtypes)]
        return (None, dx, db.view(ctx.bshape).to(ctx.bdtype), *gws)


class BoundaryLearnedConvolution2D(nn.Module):
    """Same constructor, sub-modules and state_dict keys as the reference (nine `nn.Conv2d` / `SymmetricConv2d` banks with
    bias=False and 'valid' padding, `learnable_bias` [1, c_o, 1, 1])."""

    def __init__(self, c_i, c_o, k, stride=1, use_symm=False):
        super().__init__()
        if k not in (3, 5) or stride != 1:
            raise NotImplementedError("HIP BoundaryLearnedConvolution2D supports 3x3 / 5x5 kernels, stride 1")
        self.c_i, self.c_o, self.k, self.use_symm = c_i, c_o, k, use_symm
        h_s = int(c_o / 4) if c_o > 4 else int(c_o / 2)
        self._sym_h = h_s if use_symm else 0
        for name in BANKS:
            if use_symm:
                mod = SymmetricConv2d(c_i, c_o, k, bias=False, padding="valid", symmetry={"h": h_s, "v": 0, "hv": 0})
            else:
                mod = nn.Conv2d(in_channels=c_i, out_channels=c_o, kernel_size=k, padding="valid", bias=False)
            setattr(self, name, mod)
        self.learnable_bias = nn.Parameter(torch.zeros(1, c_o, 1, 1))
        self._precision = os.environ.get("MANTLE_PRECISION", "fp32")
        self._plans, self._version = {}, 0

    def set_precision(self, precision: str):
        if precision not in _DT:
            raise ValueError("precision must be 'fp32' or 'bf16'")
        self._precision = precision
        return self

    def _plan(self, N, H, W, device):
        key = (N, H, W, self._precision, str(device))
        p = self._plans.get(key)
        if p is None:
            L.load()
            p = self._plans[key] = _Plan(N, H, W, self.c_i, self.c_o, self.k, self._sym_h, self._precision, device)
        return p

    def forward(self, x, bc_x=1, bc_y=1):
        if bc_x != 1 or bc_y != 1:
            raise NotImplementedError("bc_x / bc_y > 1 (field-growing strips of the Unet's first layer) are not implemented")
        return _LearnedConvFn.apply(self, x, self.learnable_bias, *[getattr(self, n).weight for n in BANKS])

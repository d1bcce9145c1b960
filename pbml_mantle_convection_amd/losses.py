"""Fused training loss on MI355X: Trainer.loss_fn / get_loss arithmetic (reference
multigpu.py:122-134, 250-305) plus the build-defined Stokes momentum residual, forward AND
backward in one pass over the fields (libmantle_hip: mc_loss_* / mc_momentum_* / mc_advect_loss*; the curl heads are
launched by heads.CurlHead).  What a loss object launches is decided once, in its constructor (`LossPlan`; DESIGN.md §1
"The loss's plan and routes").

`StokesLoss.evaluate` works on raw device buffers (used by the fused trainer, graph-capturable);
`StokesLoss.__call__` is the autograd-visible form used by Trainer.get_loss.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from . import _lib as L
from .heads import BLURR_NEEDS_FLUIDNET, CurlHead, HeadForm

FUSED_LOSS = os.environ.get("MANTLE_FUSED_LOSS", "1") != "0"      # mc_loss_fused instead of mc_loss_fwd_bwd + mc_momentum_*

OUT_NAMES = ("loss", "loss_true_u", "loss_true_v", "loss_p", "loss_T", "mass", "momentum", "_")


def _f32(t):
    """t as a contiguous f32 tensor (t itself when it is one)."""
    return t if (t.dtype is torch.float32 and t.is_contiguous()) else t.float().contiguous()


class LossRoute(enum.Enum):
    FUSED = "fused"        # mc_loss_fused: every term in one launch, from y's planes or the last convolution's CB8 output
    SPLIT = "split"        # [head.forward] mc_loss_fwd_bwd [mc_advect_loss_dt, mc_advect_loss] [mc_momentum_*] [head.backward]


class Zero(enum.Enum):
    ALWAYS = "always"                              # the wall heads add into channels 0 (and 1) of gy
    EXTRA_CHANNELS_ONLY = "extra"                  # the launches write every plane the loss reads: zeros for further channels only


HEAD = "head"              # a channel-map entry: the term reads the head's plane, not a channel of y


@dataclass(frozen=True, slots=True)
class LossPlan:
    route: LossRoute
    head: Optional[CurlHead]
    chan: Tuple[Union[int, str, None], ...]        # the channel map, for (u, v, T, p): a channel of y and gy, HEAD, or None = no term
    ct: int                                        # truth channels
    zero: Zero                                     # when gy is zeroed before the launches
    needs: frozenset                               # of "yc", "paras", "scaler", "advect": the optional inputs evaluate reads


class StokesLoss:
    def __init__(self, p_pred: bool, loss_type: str, loss_scale: bool = False, loss_derivative: bool = False,
                 norm: str = "l1", lambda_mom: float = 0.0, inv_h: float = 126.0, ra: float = 1.0,
                 a_bound: float = 10.0, t_grad: bool = True, has_T: bool = True, curl_valid: bool = False,
                 advect_cn: Optional[float] = None, blurr: bool = False):
        if loss_type not in L.LOSS_TYPES:
            raise ValueError(f"loss_type must be one of {list(L.LOSS_TYPES)}")
        if norm not in ("l1", "l2"):
            raise ValueError("norm must be 'l1' (reference) or 'l2'")
        self.p_pred, self.loss_type = bool(p_pred), loss_type
        self.loss_scale, self.loss_derivative = bool(loss_scale), bool(loss_derivative)
        self.norm, self.lambda_mom, self.inv_h, self.ra = norm, float(lambda_mom), float(inv_h), float(ra)
        self.a_bound, self.t_grad = float(a_bound), bool(t_grad)
        # has_T = False: FluidNet family (reference get_loss, multigpu.py:138-195): outputs (u, v[, p]) / (streamfunction[, p]),
        # truth (u, v[, p]), no temperature term, scaled pressure loss
        self.has_T = bool(has_T)
        if not self.has_T and self.lambda_mom != 0.0:
            raise ValueError("the momentum residual needs the temperature output (Unet); use lambda_mom = 0 with has_T = False")
        # curl_valid: FluidNet (reference pytorch_networks_convae.py:1681-1697): the network output is the streamfunction on the
        # grown (H+2) x (W+2) field and u, v are its plain centred differences on the H x W grid of the truth
        # (heads.HeadForm.VALID)
        self.curl_valid = bool(curl_valid)
        if self.curl_valid and (loss_type != "curl" or self.has_T or self.p_pred):
            raise ValueError("curl_valid is FluidNet's head: loss_type 'curl', has_T = False, p_pred = False")
        # advect_cn: the reference's `-ad 1` (DESIGN.md §9 "Advection loss"): a temperature term from ONE ADNet step of the
        # predicted and of the true velocity on the item's own temperature, at the CFL step of the true velocity with
        # CN_max = advect_cn (mc_advect_loss_dt -> mc_advect_loss after mc_loss_fwd_bwd)
        self.advect_cn = None if advect_cn is None else float(advect_cn)
        if self.advect_cn is not None and self.has_T:
            raise ValueError("advect_cn is the FluidNet family's temperature term: it needs has_T = False (a Unet predicts T itself)")
        if self.advect_cn is not None and not self.advect_cn > 0.0:
            raise ValueError(f"advect_cn (the ADNet's CN_max) must be > 0, got {advect_cn}")
        # blurr: the reference's `-blurr 1` for the FluidNet family (DESIGN.md §9 "Blurred streamfunction"): u, v are the curl of
        # the streamfunction's 3 x 3 box mean; the mean sits inside the head's launches
        self.blurr = bool(blurr)
        if self.blurr and (loss_type != "curl" or self.has_T):
            raise ValueError(BLURR_NEEDS_FLUIDNET)
        self.plan = self._make_plan()
        self._shape, self._frozen = None, False
        self.gsum_blocks, self.gsum_part = 0, None

    def _make_plan(self) -> LossPlan:
        """Everything evaluate() decides: it depends on the constructor's arguments and FUSED_LOSS alone, never on the shape."""
        t = 1 if self.has_T else 0
        ct = (3 if self.p_pred else 2) + t

        def p(k):                                  # the pressure channel follows the channels the other terms read
            return k if self.p_pred else None
        needs = frozenset((("yc", "paras", "scaler") if self.lambda_mom != 0.0 else ())
                          + (("advect", "scaler") if self.advect_cn is not None else ()))
        if self.loss_type == "curl":
            # channel 0 = streamfunction, then T (Unet, reference pytorch_networks_convae.py:2038-2049), then p (:1360-1369)
            form = HeadForm.VALID if self.curl_valid else HeadForm.WALL_T if self.has_T else HeadForm.WALL
            return LossPlan(LossRoute.SPLIT, CurlHead(form, self.blurr, self.a_bound), (HEAD, HEAD, HEAD if self.has_T else None,
                            p(1 + t)), ct, Zero.EXTRA_CHANNELS_ONLY if self.curl_valid else Zero.ALWAYS, needs)
        # channels u, v, T, p (Unet, :2026-2036) or u, v, p (NewFluidNet 'mae' / 'mass', :1348-1358)
        route = LossRoute.FUSED if FUSED_LOSS and self.has_T else LossRoute.SPLIT
        return LossPlan(route, None, (0, 1, 2 if self.has_T else None, p(2 + t)), ct, Zero.EXTRA_CHANNELS_ONLY, needs)

    # ------------------------------------------------------------------
    @property
    def needs(self):
        """Which of yc, paras, scaler and advect evaluate() reads (a frozenset of those names)."""
        return self.plan.needs

    def freeze(self):
        """Pin the buffers: a captured HIP graph holds their device pointers (see Engine.freeze)."""
        self._frozen = True

    def unplanned_copy(self):
        """The same configuration and plan with no buffers and not frozen (for a batch of another shape)."""
        lo = StokesLoss(self.p_pred, self.loss_type, self.loss_scale, self.loss_derivative, self.norm, self.lambda_mom, self.inv_h,
                        self.ra, self.a_bound, self.t_grad, self.has_T, self.curl_valid, self.advect_cn, self.blurr)
        lo.plan = self.plan
        return lo

    def _alloc(self, N, Cc, H, W, dev):
        if self._shape == (N, Cc, H, W, str(dev)):
            return
        if self._frozen:
            raise RuntimeError(f"this loss object is pinned to shape {self._shape[:4]} by a captured HIP graph; got {(N, Cc, H, W)}")
        f32 = dict(dtype=torch.float32, device=dev)
        head = self.plan.head
        self.sums = torch.zeros(L.LOSS_SLOTS, dtype=torch.float64, device=dev)
        self.out8 = torch.zeros(8, **f32)
        self.mm = torch.zeros((N, 3, 2), **f32)
        Hy, Wy = (H + 2, W + 2) if self.curl_valid else (H, W)     # (the gradient w.r.t. the grown field)
        self.gy = torch.zeros((N, Cc, Hy, Wy), **f32)
        if head is not None:
            self.cu, self.cv, self.cT = (torch.empty((N, H, W), **f32) for _ in range(3))
            self.gcu, self.gcv, self.gcT = (torch.empty((N, H, W), **f32) for _ in range(3))
            self.curl_ws = torch.empty(head.ws_floats(N, H, W), **f32) if head.ws_floats(N, H, W) else None
        self.gsum_blocks, self.gsum_part = 0, None
        if self.fusable() and Cc <= 4:
            # per-block spatial sums of the gradient planes (the adjoint of the network's mean subtraction takes its means
            # from them: Engine.backward(gsum=...))
            self.gsum_blocks = int(L.call("mc_loss_fused_blocks", N, H, W))
            self.gsum_part = torch.zeros((N, self.gsum_blocks, 4), **f32)
        if self.lambda_mom != 0.0 and not self.fusable():         # (the one-launch form keeps S_x, S_y and eta in LDS)
            self.sx, self.sy, self.eta = (torch.empty((N, H, W), **f32) for _ in range(3))
        if self.advect_cn is not None:
            self.adv_dt = torch.zeros(N, **f32)
            self.adv_ws = torch.zeros(L.ADVECT_WS_PER_ITEM * N, dtype=torch.int32, device=dev)
        # what the shape fixes for every later call: mc_loss_desc (t_grad = -2: the temperature term is the advection step's),
        # the planes of gy under the channel map, and whether gy is zeroed
        self._desc = L.LossDesc(N, H, W, int(self.p_pred), L.LOSS_TYPES[self.loss_type], int(self.loss_scale),
                                int(self.loss_derivative), int(self.norm == "l2"), self.lambda_mom, self.inv_h, self.ra,
                                int(self.t_grad) if self.has_T else (-1 if self.advect_cn is None else -2))
        self._plane = Hy * Wy
        self._src_head = (self.cu, self.cv, self.cT) if head is not None else None
        self._grad = self._planes(self.gy.data_ptr(), self._plane, (self.gcu, self.gcv, self.gcT) if head is not None else None)
        self._zero_gy = self.plan.zero is Zero.ALWAYS or Cc > self.channels_needed()
        self._shape = (N, Cc, H, W, str(dev))

    def channels_needed(self):
        return (1 if self.loss_type == "curl" else 2) + int(self.has_T) + int(self.p_pred)

    def gradient_sums(self):
        """(per-block sums [N, blocks, 4], blocks) of the gradient planes written by the last evaluate(), or None."""
        return None if self.gsum_part is None else (self.gsum_part, self.gsum_blocks)

    def fusable(self):
        """One-launch form (mc_loss_fused): the Unet branch without the curl head (and FUSED_LOSS when the loss was built)."""
        return self.plan.route is LossRoute.FUSED

    def _validate(self, y, uvp, cb8, advect):
        """(N, Cc, H, W, device, uvp, advect) with uvp and advect = (x, scaler) as contiguous f32, or the caller's error."""
        L.require_cuda(uvp, "uvp")
        if cb8 is not None:
            if self.plan.route is not LossRoute.FUSED:
                raise RuntimeError("the CB8 form needs the one-launch loss (Unet branch without the curl head)")
            N, Cc, H, W = cb8[3]
            dev = cb8[0].device
        else:
            L.require_cuda(y, "network output")
            if y.dtype != torch.float32 or not y.is_contiguous():
                raise RuntimeError("y must be contiguous f32")
            N, Cc, H, W = y.shape
            if self.plan.head is not None:
                H, W = self.plan.head.out_hw(H, W)
            dev = y.device
        uvp = _f32(uvp)
        if Cc < self.channels_needed():
            raise ValueError(f"network output has {Cc} channels, loss needs {self.channels_needed()}")
        if tuple(uvp.shape) != (N, self.plan.ct, H, W):
            raise ValueError(f"uvp must be [{N},{self.plan.ct},{H},{W}], got {tuple(uvp.shape)}")
        if (advect is not None) != ("advect" in self.plan.needs):
            raise ValueError("advect=(x, scaler) goes with a loss built with advect_cn, and a loss built with advect_cn needs it")
        if advect is not None:
            ax, asc = advect
            L.require_cuda(ax, "advect x")
            L.require_cuda(asc, "advect scaler")
            if ax.dim() != 4 or ax.shape[0] != N or ax.shape[1] < 7 or tuple(ax.shape[2:]) != (H, W):
                raise ValueError(f"advect x must be [{N}, >= 7, {H}, {W}], got {tuple(ax.shape)}")
            if asc.numel() != N:
                raise ValueError(f"advect scaler must hold {N} values, got {tuple(asc.shape)}")
            advect = _f32(ax), _f32(asc)
        return N, Cc, H, W, dev, uvp, advect

    def _mom_inputs(self, yc, paras, scaler, N, H, W):
        """The momentum term's (yc [H, W], paras [N, 3], scaler [N]) as contiguous f32; Nones without the term."""
        if "yc" not in self.plan.needs:
            return None, None, None
        if yc is None or paras is None or scaler is None:
            raise ValueError("the momentum term needs yc [H,W], paras [N,3] and scaler [N]")
        # ONE depth grid for the whole batch (all samples of a data set share the mesh; a loader delivers it per sample):
        # Trainer checks once, outside the captured step, that the rows are equal (Trainer._check_single_mesh)
        return _f32(yc.reshape(-1, H, W)[0]), _f32(paras.reshape(N, 3)), _f32(scaler.reshape(N))

    def _planes(self, base, plane, head_planes):
        """(u, v, T, p) device pointers under the plan's channel map: channel k of the f32 tensor at `base` whose channels
        are `plane` floats apart, or the head's plane of that term."""
        return [None if c is None else head_planes[i].data_ptr() if c is HEAD else base + 4 * c * plane
                for i, c in enumerate(self.plan.chan)]

    def evaluate(self, y: Optional[torch.Tensor], uvp: torch.Tensor, yc: Optional[torch.Tensor] = None,
                 paras: Optional[torch.Tensor] = None, scaler: Optional[torch.Tensor] = None, cb8=None, advect=None):
        """y: network output [N, C, H, W] f32 (Unet.features / ConvAE output; [N, C, H + 2, W + 2] with curl_valid);
        uvp: truth [N, 2|3|4, H, W] f32.  Returns (out8, gy): out8 = (loss, true_u, true_v, loss_p, loss_T, mass,
        momentum, 0) on device; gy = d(loss)/d(y).
        cb8 (only with `fusable()`): (buf, mean, crop, (N, C, H, W)) -- the last convolution's f32 output in the CB8 layout
        [N][ceil(C / 8)][H][W + 2 crop][8] and its per-(sample, channel) spatial means; y is not read then (may be None).
        advect (with `advect_cn`, and only then): (x, scaler) -- the batch's input x [N, >= 7, H, W] f32 = (xc/4, yc/4,
        log10 eta/8, nd0, nd1, nd2, T, ...) and the velocity scale [N]; out8[4] is then the advection step's temperature error."""
        N, Cc, H, W, dev, uvp, advect = self._validate(y, uvp, cb8, advect)
        mom = self._mom_inputs(yc, paras, scaler, N, H, W)
        self._alloc(N, Cc, H, W, dev)
        plan, st, d = self.plan, L.stream(), self._desc
        self.sums.zero_()
        if self.loss_scale:
            L.call("mc_loss_minmax", L.ptr(uvp), N, plan.ct, H, W, L.ptr(self.mm), st)
        if self._zero_gy:
            self.gy.zero_()
        plane = self._plane
        src = None if cb8 is not None else self._planes(y.data_ptr(), plane, self._src_head)
        if plan.route is LossRoute.FUSED:
            self._launch_fused(d, src, self._grad, Cc * plane, cb8, uvp, mom, st)
        else:
            self._launch_split(d, y.data_ptr(), src, self._grad, Cc, plane, uvp, mom, advect, st)
        L.call("mc_loss_finalize", C.byref(d), L.ptr(self.sums), L.ptr(self.out8), st)
        return self.out8, self.gy

    def _launch_fused(self, d, src, grad, stride, cb8, uvp, mom, st):
        gu, gv, gT, gp = grad
        if cb8 is not None:
            buf, mean, crop, (_, Cc, _, W) = cb8
            source = (None, None, None, None, 0, 0, L.ptr(buf), W + 2 * crop, crop, L.ptr(mean), Cc)
        else:
            u, v, T, p = src
            source = (u, v, p, T, stride, stride, None, 0, 0, None, 0)
        yc, paras, scaler = mom
        L.call("mc_loss_fused", C.byref(d), *source, L.ptr(uvp), L.ptr(self.mm), L.ptr(yc), L.ptr(paras), L.ptr(scaler),
               L.ptr(self.sums), gu, gv, gp, gT, stride, stride, L.ptr(self.gsum_part), st)

    def _launch_split(self, d, y_ptr, src, grad, Cc, plane, uvp, mom, advect, st):
        (u, v, T, p), (gu, gv, gT, gp) = src, grad
        head, (N, H, W) = self.plan.head, (d.n, d.h, d.w)
        pbs, ppbs = (H * W if head is not None else Cc * H * W), Cc * H * W     # batch strides of u, v, T and of p
        if head is not None:
            head.forward(y_ptr, Cc * plane, N, H, W, u, v, T, st)
        L.call("mc_loss_fwd_bwd", C.byref(d), u, v, p, T, pbs, ppbs, L.ptr(uvp), L.ptr(self.mm), L.ptr(self.sums), gu,
               gv, gp, gT, st)
        if advect is not None:
            ax, asc = advect
            L.call("mc_advect_loss_dt", L.ptr(uvp), self.plan.ct, L.ptr(ax), int(ax.shape[1]), L.ptr(asc), N, H, W,
                   self.advect_cn, L.ptr(self.adv_ws), L.ptr(self.adv_dt), st)
            L.call("mc_advect_loss", C.byref(d), u, v, pbs, L.ptr(uvp), L.ptr(ax), int(ax.shape[1]), L.ptr(asc),
                   L.ptr(self.adv_dt), L.ptr(self.sums), gu, gv, st)
        if self.lambda_mom != 0.0:
            yc, paras, scaler = mom
            L.call("mc_momentum_residual", C.byref(d), u, v, p, T, pbs, ppbs, L.ptr(yc), L.ptr(paras), L.ptr(scaler),
                   L.ptr(self.sums), L.ptr(self.sx), L.ptr(self.sy), L.ptr(self.eta), st)
            L.call("mc_momentum_adjoint", C.byref(d), T, pbs, ppbs, L.ptr(self.eta), L.ptr(paras), L.ptr(scaler),
                   L.ptr(self.sx), L.ptr(self.sy), gu, gv, gp, gT, st)
        if head is not None:
            head.backward(gu, gv, gT, y_ptr, Cc * plane, N, H, W, self.gy.data_ptr(), Cc * plane, L.ptr(self.curl_ws), st)

    def __call__(self, y, uvp, yc=None, paras=None, scaler=None, advect=None):
        """Autograd-visible: returns out8 whose element 0 back-propagates d(loss)/dy into y."""
        return _LossFn.apply(self, y, uvp, yc, paras, scaler, advect)


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loss_obj, y, uvp, yc, paras, scaler, advect=None):
        out8, gy = loss_obj.evaluate(y.contiguous(), uvp, yc, paras, scaler, advect=advect)
        ctx.gy = gy.clone()
        return out8.clone()

    @staticmethod
    def backward(ctx, gout):
        return None, ctx.gy * gout[0], None, None, None, None, None

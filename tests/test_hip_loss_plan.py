"""GPU: what `StokesLoss.evaluate` decides on the host -- the route, the head, the channel map, the strides, the zeroing rule
-- on real memory, one configuration per row family of tests/loss_trace.py at N = 2 and the smallest shapes at which a plane
pointer or a stride can go wrong.

(a) evaluate against the same launches issued by hand through `L.call` (the heads through `heads.CurlHead`), channel planes
    written out as numbers: gy bit for bit; out8 as test_hip_train.test_one_launch_loss_equals_the_three_kernels compares it
    (atol 1e-7, rtol 1e-6), because the reducing kernels add into f64 sums with atomics.
(b) a second evaluate after gy, sums, out8 and every buffer that `_alloc` leaves uninitialised (the head's planes and their
    gradients, curl_ws, sx, sy, eta) were filled with NaN: the same gy bit for bit, the same out8 within that tolerance.  A
    wrong zeroing rule or a plane left unwritten fails here.  mm, gsum_part, adv_dt and adv_ws are zero-initialised once
    and stay out of the set: that their kernels rewrite them in full is not established."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import advect_loss_ref as A
import fields
import loss_trace as LT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, LAM, CN, A_BOUND = 2, 1e-6, 2e4, 10.0
ATOL, RTOL = 1e-7, 1e-6
UNINITIALISED = ("cu", "cv", "cT", "gcu", "gcv", "gcT", "curl_ws", "sx", "sy", "eta")

# kw: StokesLoss arguments; fused: losses.FUSED_LOSS at construction; head: the CurlHead form; u, v, T, p: the channel of y
# (and of gy) the term reads, absent = from the head's planes or not there at all
FAMILIES = {
    "unet fused": dict(kw=dict(p_pred=True, loss_type="mass", lambda_mom=LAM), fused=True, u=0, v=1, T=2, p=3),
    "unet cb8": dict(kw=dict(p_pred=True, loss_type="mass", lambda_mom=LAM), fused=True, cb8=True, u=0, v=1, T=2, p=3),
    "unet split": dict(kw=dict(p_pred=True, loss_type="mass", lambda_mom=LAM), fused=False, u=0, v=1, T=2, p=3),
    "unet curl": dict(kw=dict(p_pred=True, loss_type="curl", lambda_mom=LAM), head="WALL_T", p=2),
    "newfluidnet mass": dict(kw=dict(p_pred=True, loss_type="mass", has_T=False, advect_cn=CN), u=0, v=1, p=2),
    "newfluidnet curl": dict(kw=dict(p_pred=True, loss_type="curl", has_T=False, advect_cn=CN), head="WALL", p=1),
    "fluidnet": dict(kw=dict(p_pred=False, loss_type="curl", has_T=False, curl_valid=True, advect_cn=CN), head="VALID"),
}
BLURRED = ("newfluidnet curl", "fluidnet")
# 5 x 5: the minimum; 9 x 66: both halo columns across the 64-pixel seam, one row past the 8-row tile; the last with one
# output channel more than the loss reads (the zeroing rule); 17 x 65, blurred heads: one past BT_Y = 16 and BT_X = 64
CASES = ([(f, h, w, False, 0) for f in FAMILIES for (h, w) in ((5, 5), (9, 66))] + [(f, 9, 66, False, 1) for f in FAMILIES]
         + [(f, 17, 65, True, s) for f in BLURRED for s in (0, 1)])
IDS = [f"{f}-{h}x{w}{'-blurr' if b else ''}{'-spare' if s else ''}" for f, h, w, b, s in CASES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV).contiguous()


def close(a, b, what):
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    err = np.abs(a - b)
    assert (err <= ATOL + RTOL * np.abs(b)).all(), f"{what}: max err {err.max():.3e}, ref max {np.abs(b).max():.3e}"


@functools.lru_cache(maxsize=None)
def inputs(family, H, W, spare):
    """The device tensors of a case, built once and never written: y [N, Cc, H (+2), W (+2)], uvp, (yc, paras, scaler) or
    Nones, advect (x, scaler) or None."""
    f = FAMILIES[family]
    kw, g = f["kw"], 2 if f.get("head") == "VALID" else 0
    a = fields.smooth_field(N, H + g, W + g, 11)
    if kw.get("has_T", True):
        u, v = (fields.smooth_field(N, H, W, 12 + i, noise=0.01) for i in range(2))
        p, T = fields.smooth_field(N, H, W, 14, amp=0.5), fields.temperature_field(N, H, W, 15) * 1.3 - 0.1
        uvp = np.stack([fields.smooth_field(N, H, W, 16), fields.smooth_field(N, H, W, 17),
                        fields.smooth_field(N, H, W, 18, amp=0.5), fields.temperature_field(N, H, W, 19)], 1)
        paras = fields.sim_parameters(N, 5)
        paras[:, 1] = 10.0 ** np.array([2.0, 3.0])
        mom = (dev(np.broadcast_to(np.linspace(0, 1, H)[:, None], (H, W))), dev(paras), dev(np.array([30.0, 80.0])))
        advect = None
        chans = [a, T, p] if "head" in f else [u, v, T, p]
    else:
        c = A.case(N, H, W)
        uvp = c["uvp"][:, :3 if kw["p_pred"] else 2]
        mom, advect = (None, None, None), (dev(c["x"]), dev(c["s"]))
        chans = {None: [c["up"], c["vp"], c["pp"]], "WALL": [a, c["pp"]], "VALID": [a]}[f.get("head")]
    chans += [fields.smooth_field(N, H + g, W + g, 20)] * spare
    return dev(np.stack(chans, 1)), dev(uvp), mom, advect


def cb8_of(y):
    """y in the CB8 layout the engine's last convolution leaves: (buf, mean, crop, shape) and the planes the kernel sees."""
    n, c, H, W = y.shape
    crop = LT.CROP
    gen = torch.Generator(device=DEV).manual_seed(3)
    mean = torch.randn(n, c, device=DEV, generator=gen)
    buf = torch.randn(n, 1, H, W + 2 * crop, 8, device=DEV, generator=gen)      # crop columns, spare channels: garbage
    buf[:, 0, :, crop:crop + W, :c] = (y + mean[:, :, None, None]).permute(0, 2, 3, 1)
    y_eff = buf[:, 0, :, crop:crop + W, :c].permute(0, 3, 1, 2).contiguous() - mean[:, :, None, None]
    return (buf, mean, crop, (n, c, H, W)), y_eff


def build(family, blurr):
    f = FAMILIES[family]
    with LT.fused_loss(f.get("fused")) as losses:
        return losses.StokesLoss(a_bound=A_BOUND, **f["kw"], **({"blurr": True} if blurr else {}))


def evaluate(loss, family, y, uvp, mom, advect):
    f = FAMILIES[family]
    with LT.fused_loss(f.get("fused")):
        if f.get("cb8"):
            return loss.evaluate(None, uvp, *mom, cb8=cb8_of(y)[0])
        return loss.evaluate(y, uvp, *mom, advect=advect)


def by_hand(family, blurr, y, uvp, mom, advect):
    """The launches of the family written out: (out8, gy) in buffers of its own."""
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import heads
    f = FAMILIES[family]
    kw = f["kw"]
    n, Cc, Hy, Wy = y.shape
    g = 2 if f.get("head") == "VALID" else 0
    H, W = Hy - g, Wy - g
    HW, stride = H * W, Cc * Hy * Wy
    has_T = kw.get("has_T", True)
    f32 = dict(dtype=torch.float32, device=DEV)
    sums, out8 = torch.zeros(L.LOSS_SLOTS, dtype=torch.float64, device=DEV), torch.zeros(8, **f32)
    mm, gy = torch.zeros((n, 3, 2), **f32), torch.zeros((n, Cc, Hy, Wy), **f32)
    d = L.LossDesc(n, H, W, int(kw["p_pred"]), L.LOSS_TYPES[kw["loss_type"]], 0, 0, 0, kw.get("lambda_mom", 0.0), 126.0, 1.0,
                   1 if has_T else -2)
    st = L.stream()

    def plane(t, name):
        return t.data_ptr() + 4 * f[name] * Hy * Wy if name in f else None
    if f.get("fused"):
        blocks = int(L.call("mc_loss_fused_blocks", n, H, W))
        part = torch.zeros((n, blocks, 4), **f32) if Cc <= 4 else None
        src = [None, None, None, None, 0, 0, None, 0, 0, None, 0]
        if f.get("cb8"):
            (buf, mean, crop, _), _ = cb8_of(y)
            src[6:] = [L.ptr(buf), W + 2 * crop, crop, L.ptr(mean), Cc]
        else:
            src[:6] = [plane(y, "u"), plane(y, "v"), plane(y, "p"), plane(y, "T"), stride, stride]
        L.call("mc_loss_fused", C.byref(d), *src, L.ptr(uvp), L.ptr(mm), *(L.ptr(t) for t in mom), L.ptr(sums), plane(gy, "u"),
               plane(gy, "v"), plane(gy, "p"), plane(gy, "T"), stride, stride, L.ptr(part), st)
        L.call("mc_loss_finalize", C.byref(d), L.ptr(sums), L.ptr(out8), st)
        return out8, gy
    u, v, T, p, pbs = plane(y, "u"), plane(y, "v"), plane(y, "T"), plane(y, "p"), stride
    gu, gv, gT, gp = plane(gy, "u"), plane(gy, "v"), plane(gy, "T"), plane(gy, "p")
    if "head" in f:
        head = heads.CurlHead(heads.HeadForm[f["head"]], blurr, A_BOUND)
        hu, hv, hT, hgu, hgv, hgT = (torch.empty((n, H, W), **f32) for _ in range(6))
        ws = torch.empty(max(head.ws_floats(n, H, W), 1), **f32)
        with_T = f["head"] == "WALL_T"
        head.forward(y.data_ptr(), stride, n, H, W, L.ptr(hu), L.ptr(hv), L.ptr(hT) if with_T else None, st)
        u, v, T, pbs = L.ptr(hu), L.ptr(hv), L.ptr(hT) if with_T else None, HW
        gu, gv, gT = L.ptr(hgu), L.ptr(hgv), L.ptr(hgT) if with_T else None
    L.call("mc_loss_fwd_bwd", C.byref(d), u, v, p, T, pbs, stride, L.ptr(uvp), L.ptr(mm), L.ptr(sums), gu, gv, gp, gT, st)
    if advect is not None:
        ax, asc = advect
        adv_dt, adv_ws = torch.zeros(n, **f32), torch.zeros(L.ADVECT_WS_PER_ITEM * n, dtype=torch.int32, device=DEV)
        L.call("mc_advect_loss_dt", L.ptr(uvp), int(uvp.shape[1]), L.ptr(ax), 7, L.ptr(asc), n, H, W, CN, L.ptr(adv_ws),
               L.ptr(adv_dt), st)
        L.call("mc_advect_loss", C.byref(d), u, v, pbs, L.ptr(uvp), L.ptr(ax), 7, L.ptr(asc), L.ptr(adv_dt), L.ptr(sums), gu, gv,
               st)
    if kw.get("lambda_mom"):
        yc, paras, scaler = mom
        sx, sy, eta = (torch.empty((n, H, W), **f32) for _ in range(3))
        L.call("mc_momentum_residual", C.byref(d), u, v, p, T, pbs, stride, L.ptr(yc), L.ptr(paras), L.ptr(scaler), L.ptr(sums),
               L.ptr(sx), L.ptr(sy), L.ptr(eta), st)
        L.call("mc_momentum_adjoint", C.byref(d), T, pbs, stride, L.ptr(eta), L.ptr(paras), L.ptr(scaler), L.ptr(sx), L.ptr(sy),
               gu, gv, gp, gT, st)
    if "head" in f:
        head.backward(gu, gv, gT, y.data_ptr(), stride, n, H, W, gy.data_ptr(), stride, L.ptr(ws), st)
    L.call("mc_loss_finalize", C.byref(d), L.ptr(sums), L.ptr(out8), st)
    return out8, gy


@pytest.mark.parametrize("family,H,W,blurr,spare", CASES, ids=IDS)
def test_evaluate_equals_the_launches_by_hand(family, H, W, blurr, spare):
    y, uvp, mom, advect = inputs(family, H, W, spare)
    loss = build(family, blurr)
    out8, gy = evaluate(loss, family, y, uvp, mom, advect)
    ref8, refg = by_hand(family, blurr, y, uvp, mom, advect)
    assert bool(torch.isfinite(refg).all()) and float(refg.abs().max()) > 0.0
    assert gy.shape == refg.shape and torch.equal(gy, refg), float((gy - refg).abs().max())
    close(out8, ref8, "out8")


@pytest.mark.parametrize("family,H,W,blurr,spare", CASES, ids=IDS)
def test_second_evaluate_ignores_poisoned_buffers(family, H, W, blurr, spare):
    y, uvp, mom, advect = inputs(family, H, W, spare)
    loss = build(family, blurr)
    out8, gy = (t.clone() for t in evaluate(loss, family, y, uvp, mom, advect))
    assert bool(torch.isfinite(gy).all()) and bool(torch.isfinite(out8).all()) and float(gy.abs().max()) > 0.0
    poisoned = [loss.gy, loss.sums, loss.out8] + [t for t in (getattr(loss, n, None) for n in UNINITIALISED) if t is not None]
    for t in poisoned:
        t.fill_(float("nan"))
    again8, againg = evaluate(loss, family, y, uvp, mom, advect)
    assert torch.equal(againg, gy), f"gy differs after poisoning {len(poisoned)} buffers"
    close(again8, out8, "out8")

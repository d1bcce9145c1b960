"""Cases, the f64 reference, derived bounds and kink rules for the advection loss (csrc/advect_loss.hip, DESIGN.md §9
"Advection loss"): tests/test_advect_loss_ref_host.py on the CPU, tests/test_hip_advect_loss.py and
tests/test_hip_advect_loss_net.py on the GPU.

The reference composes the oracle: oracle.ref_cpu.adnet_step twice with the GIVEN dt [N] (once with the predicted, once with the
true velocity, both times on the item's own temperature and grid, RaQ = 0) and oracle.ref_cpu.get_loss_fluidnet, under torch
autograd in f64.  `direct()` restates e, the upwind differences and the sum of magnitudes by index; the host test holds it
against the composition and against a 5 x 5 case computed by hand.

Bounds.  U = 2^-24.  The library is built with -ffp-contract=off, so every operation rounds once.  X = 4 x[0] and Y = 4 x[1] are
exact, so a spacing and a temperature difference carry one rounding each RELATIVE TO THEIR RESULT (their operands are inputs):

  K_E = 8     e = dt ((-uu DxP - vv DyP) - (-ur DxT - vr DyT)): an upwind difference is (difference / difference): 3 roundings;
              uu = s u: 1; their product: 5; the sum of two products: 6; the difference of the two sums: 7; x dt: 8 -- times
              the sum of magnitudes M_e = dt (|uu DxP| + |vv DyP| + |ur DxT| + |vr DyT|)
  K_G = 8     an increment q (-DxP): cg = dt s / (k (N HW)) is 3 roundings on its longest chain (N HW, x k, the quotient),
              (de w) cg one more, DxP 3, the product 1 -- relative to the increment.  With l2, de = 2 e carries e's error:
              + 2 B_e w cg |DxP|.  The read-modify-write rounds once more, relative to the stored value: + U (|g0| + |g0 + ref|)
  sums        a term |e| w (w in {1, 2, 3}: exact) is off by B_e w; with l2, e e w by (2 |e| B_e + B_e^2 + U e^2) w.  A thread adds
              `adds` terms into its f32 partial: + adds U (the sum); threads, waves and blocks combine in f64

Kink rules (the issue's): a pixel is left out of a gradient comparison where |e_ref| < 1e-4 max|e_ref| (the sign of e) or where
0 < |s u_p| < 1e-4 max|s u_p| (the same for v); the maxima are taken per item (the items' time steps, and with them their e,
differ by orders of magnitude: the batch-wide maximum would leave out more).  The host test asserts, on the reference alone, that the excluded share is <= 1 %
and that B_e lies below the first threshold wherever a pixel is kept, so that the sign cannot differ there.
"""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fields  # noqa: E402
import step_cases as Sc  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

f64 = torch.float64
F32 = np.float32
U = 2.0 ** -24
K_E, K_G = 8, 8
KINK = 1e-4
MAX_SHARE = 0.01
CN_REF, CN_ADV = 2e4, 0.1              # the reference's ADNet(CN_max=2e4): the diffusive limit; 0.1: the advective one

# tile of k_advect_loss (rows x pixels per workgroup pass) and its launch formula, restated
TH, TW = 8, 64
# every interior pixel on a wall and both doubled columns; the column seam of a tile (remainder 6); four row seams and the
# column seam (remainders 5 and 2); tile + 1 and 2 tile - 1 in each extent
SHAPES = [(5, 5), (7, 70), (37, 66), (9, 65), (15, 127)]
BATCHES = [1, 3]


def cdiv(a, b):
    return -(-a // b)


def adds_per_thread(N, H, W):
    tiles = cdiv(W, TW) * cdiv(H, TH)
    grid = max(1, min(cdiv(1024, N), tiles))
    return (TH // 4) * cdiv(tiles, grid)


def r32(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


def item_grid(b, H, W, shared=False):
    """(xc, yc) [H, W] f32 of item b, NaN in the stored wall coordinates: 0 the stretched and sheared grid of
    tests/step_cases.py, 1 the uniform one, 2 the stretched one mirrored in both directions.  shared: item 0's for all."""
    k = 0 if shared else b % 3
    if k == 1:
        xc, yc = Sc.grid_uniform(H, W)
        xc, yc = xc.copy(), yc.copy()
        xc[:, 0] = xc[:, -1] = np.nan
        yc[0, :] = yc[-1, :] = np.nan
        return xc, yc
    xc, yc = Sc.grid_stretched(H, W)
    if k == 2:
        xc, yc = (F32(4.0) - xc[::-1, ::-1]).astype(F32), (F32(1.0) - yc[::-1, ::-1]).astype(F32)
    return xc, yc


@functools.lru_cache(maxsize=None)
def case(N, H, W, shared=False):
    """One batch of a FluidNet-family loss: x [N,7,H,W], truth uvp [N,3,H,W] (u, v, p), predictions u_p, v_p, p_p [N,H,W], scaler
    [N]; f64 numpy arrays holding f32 values.  Velocities of both signs, a stretched yc, a grid per item (unless `shared`), exact
    zeros planted in u_p and v_p (next to both side walls and across the tile seams), and with N >= 2 the LAST item's true
    velocity at rest."""
    seed = 4000 + 100 * N + 7 * H + W
    rng = np.random.RandomState(seed)
    x = np.zeros((N, 7, H, W))
    for b in range(N):
        xc, yc = item_grid(b, H, W, shared)
        x[b, 0], x[b, 1] = xc / F32(4.0), yc / F32(4.0)
        assert np.array_equal((F32(4.0) * x[b, 0].astype(F32))[:, 1:-1], xc[:, 1:-1])        # X = 4 x[0] is exact
    T = fields.temperature_field(N, H, W, seed + 3)
    T[:, 1:-1, :] += 0.05 * fields.smooth_field(N, H, W, seed + 5, amp=1.0)[:, 1:-1, :]      # (a 3-wide plume field is flat along x)
    x[:, 6] = np.clip(T, 0.0, 1.35)
    x[:, 2] = fields.smooth_field(N, H, W, seed + 6, amp=0.5) - 0.5
    x[:, 3:6] = rng.uniform(size=(N, 3, 1, 1))
    # (scaled velocities of order 1: with s of 30 .. 80 every moving item is advection-limited at CN_max = 0.1 on every grid)
    ut, vt = fields.smooth_field(N, H, W, seed + 1, amp=1.0, noise=0.01), fields.smooth_field(N, H, W, seed + 2, amp=1.0, noise=0.01)
    if N >= 2:
        ut[N - 1] = 0.0
        vt[N - 1] = 0.0
    up = ut + fields.smooth_field(N, H, W, seed + 7, amp=0.3, noise=0.1)
    vp = vt + fields.smooth_field(N, H, W, seed + 8, amp=0.3, noise=0.1)
    zeros_u = sorted({(1, 1), (H - 2, W - 2), (min(H - 2, 31), min(W - 2, 63)), (min(H - 2, 32), min(W - 2, 64)), (2, W - 2),
                      (min(H - 2, 8), min(W - 2, 3))})
    zeros_v = sorted({(1, W - 2), (H - 2, 1), (min(H - 2, 32), min(W - 2, 63)), (2, 2), (min(H - 2, 7), min(W - 2, 4))} - set(zeros_u))
    for (i, j) in zeros_u:
        up[:, i, j] = 0.0
    for (i, j) in zeros_v:
        vp[:, i, j] = 0.0
    pt = fields.smooth_field(N, H, W, seed + 9, amp=0.5)
    pp = pt + fields.smooth_field(N, H, W, seed + 10, amp=0.05, noise=0.1)
    return dict(N=N, H=H, W=W, x=r32(x), uvp=r32(np.stack([ut, vt, pt], 1)), up=r32(up), vp=r32(vp), pp=r32(pp),
                s=r32(30.0 + 50.0 * rng.uniform(size=N)), zeros_u=zeros_u, zeros_v=zeros_v)


def grid64(c):
    """(X, Y) [N, H, W] f64 with the wall coordinates written in."""
    X, Y = 4.0 * c["x"][:, 0], 4.0 * c["x"][:, 1]
    X, Y = X.copy(), Y.copy()
    X[:, :, 0], X[:, :, -1] = 0.0, 4.0
    Y[:, 0, :], Y[:, -1, :] = 0.0, 1.0
    return X, Y


# ---- the time step ---------------------------------------------------------------------------------------------------------
def dt32(c, cn):
    """dt [N] f32: the header's expression evaluated operation by operation in np.float32, per item."""
    out = np.empty(c["N"], F32)
    for b in range(c["N"]):
        X = (F32(4.0) * c["x"][b, 0].astype(F32)).astype(F32)
        X[:, 0], X[:, -1] = F32(0.0), F32(4.0)
        dx = (X[1:-1, 1:-1] - X[1:-1, :-2]).min()
        s = F32(c["s"][b])
        su, sv = s * c["uvp"][b, 0].astype(F32)[1:-1, 1:-1], s * c["uvp"][b, 1].astype(F32)[1:-1, 1:-1]
        uv = max(np.abs(su).max(), np.abs(sv).max())
        assert dx.dtype == F32 and uv.dtype == F32
        with np.errstate(divide="ignore"):
            adv = F32(0.5) * F32(cn) * dx / uv
        dx2 = dx * dx
        dif = F32(0.5) * (dx2 * dx2) / (dx2 + dx2)
        out[b] = min(adv, dif)
    return out


def dt_limits64(c, cn):
    """(advective, diffusive) limit [N] in f64; the advective one is +inf for an item at rest."""
    X, _ = grid64(c)
    dx = (X[:, 1:-1, 1:-1] - X[:, 1:-1, :-2]).min(axis=(1, 2))
    s = c["s"][:, None, None]
    uv = np.maximum(np.abs(s * c["uvp"][:, 0, 1:-1, 1:-1]).max(axis=(1, 2)), np.abs(s * c["uvp"][:, 1, 1:-1, 1:-1]).max(axis=(1, 2)))
    with np.errstate(divide="ignore"):
        return 0.5 * cn * dx / uv, 0.5 * dx ** 4 / (2.0 * dx ** 2)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def adnet_pair(c, dt, up, vp):
    """(ADNet(pred)[0], ADNet(true)[0]) [N,1,H,W]: oracle.ref_cpu.adnet_step with dt [N] given, RaQ = 0; up, vp f64 tensors."""
    N, H, W = c["N"], c["H"], c["W"]
    x, s = t64(c["x"]), t64(c["s"]).view(N, 1, 1)
    uvp = t64(c["uvp"])
    d4 = t64(dt).view(N, 1, 1, 1)
    z = torch.zeros((N, H, W), dtype=f64)

    def step(u, v):
        return O.adnet_step(torch.stack([s * u, s * v, x[:, 6], z, 4.0 * x[:, 0], 4.0 * x[:, 1]], 1), dt=d4)[0]
    return step(up, vp), step(uvp[:, 0], uvp[:, 1])


def loss_T(c, dt, up, vp, norm="l1"):
    Tp, Tt = adnet_pair(c, dt, up, vp)
    d = Tp - Tt
    return d.abs().mean() if norm == "l1" else (d * d).mean()


def term64(c, dt, norm="l1", p_pred=True):
    """The temperature term alone: (sum over the batch = loss_T N H W, d(loss_T / k)/d(u_p), d(loss_T / k)/d(v_p)), k = 4 (3)."""
    up, vp = t64(c["up"]).requires_grad_(True), t64(c["vp"]).requires_grad_(True)
    lT = loss_T(c, dt, up, vp, norm)
    k = 4.0 if p_pred else 3.0
    gu, gv = torch.autograd.grad(lT / k, (up, vp))
    return float(lT.detach()) * c["N"] * c["H"] * c["W"], gu.numpy(), gv.numpy()


def full_loss(c, dt, pred, *, p_pred, loss_type, loss_scale=False, loss_derivative=False, norm="l1"):
    """The reference's 6-tuple with the temperature term (multigpu.py:178-192): (loss_u + loss_v [+ loss_p] + loss_T) / 3 [4] + the
    mass terms, from oracle.ref_cpu.get_loss_fluidnet (whose average runs over one term less) and loss_T.  pred = (u, v, p)
    f64 tensors [N,H,W] (p None without p_pred)."""
    uvp = t64(c["uvp"])[:, :3 if p_pred else 2]
    kw = dict(p_pred=p_pred, loss_scale=loss_scale, loss_derivative=loss_derivative, norm=norm)
    with_mass = O.get_loss_fluidnet(pred, uvp, loss_type=loss_type, **kw)
    data = O.get_loss_fluidnet(pred, uvp, loss_type="mae", **kw)[0]              # (loss_u + loss_v [+ loss_p]) / k0
    k0 = 3.0 if p_pred else 2.0
    lT = loss_T(c, dt, pred[0], pred[1], norm)
    loss = (data * k0 + lT) / (k0 + 1.0) + (with_mass[0] - data)
    return loss, with_mass[1], with_mass[2], with_mass[3], lT, with_mass[5]


def direct(c, dt, norm="l1", p_pred=True):
    """By index, f64: e [N,H,W] (0 on the wall rows, the side columns repeated), B_e its bound, the weighted sum and its tolerance,
    the increments of the u and v gradient planes and the parts of their tolerances that do not depend on the prefill."""
    N, H, W = c["N"], c["H"], c["W"]
    X, Y = grid64(c)
    T = c["x"][:, 6]
    In = (slice(None), slice(1, -1), slice(1, -1))
    s = c["s"][:, None, None]
    d3 = np.asarray(dt, np.float64)[:, None, None]
    dxl, dxr = X[In] - X[:, 1:-1, :-2], X[:, 1:-1, 2:] - X[In]
    dyt, dyb = Y[In] - Y[:, :-2, 1:-1], Y[:, 2:, 1:-1] - Y[In]
    gl, gr = (T[In] - T[:, 1:-1, :-2]) / dxl, (T[:, 1:-1, 2:] - T[In]) / dxr
    gt, gb = (T[In] - T[:, :-2, 1:-1]) / dyt, (T[:, 2:, 1:-1] - T[In]) / dyb

    def up_(a, lo, hi):
        return lo * (a > 0) + hi * (a < 0)
    uu, vv, ur, vr = s * c["up"][In], s * c["vp"][In], s * c["uvp"][:, 0][In], s * c["uvp"][:, 1][In]
    DxP, DyP, DxT, DyT = up_(uu, gl, gr), up_(vv, gt, gb), up_(ur, gl, gr), up_(vr, gt, gb)
    e = d3 * ((-uu * DxP - vv * DyP) - (-ur * DxT - vr * DyT))
    Me = d3 * (np.abs(uu * DxP) + np.abs(vv * DyP) + np.abs(ur * DxT) + np.abs(vr * DyT))
    Be = K_E * U * Me
    w = np.ones((1, 1, W - 2))
    w[..., 0] += 1.0
    w[..., -1] += 1.0
    k = 4.0 if p_pred else 3.0
    cg = d3 * s / (k * N * H * W)
    if norm == "l1":
        terms, tb, de, dde = np.abs(e) * w, Be * w, np.sign(e), 0.0 * e
    else:
        terms, tb, de, dde = e * e * w, (2.0 * np.abs(e) * Be + Be * Be + U * e * e) * w, 2.0 * e, 2.0 * Be
    total = float(terms.sum())
    tol = float(tb.sum()) + adds_per_thread(N, H, W) * U * total
    q = de * w * cg
    iu, iv = np.zeros((N, H, W)), np.zeros((N, H, W))
    bu, bv = np.zeros((N, H, W)), np.zeros((N, H, W))
    iu[In], iv[In] = q * (-DxP), q * (-DyP)
    bu[In] = K_G * U * np.abs(iu[In]) + dde * w * cg * np.abs(DxP)
    bv[In] = K_G * U * np.abs(iv[In]) + dde * w * cg * np.abs(DyP)
    full = np.zeros((N, H, W))
    full[In] = e
    full[:, 1:-1, 0], full[:, 1:-1, -1] = full[:, 1:-1, 1], full[:, 1:-1, -2]
    return dict(e=full, e_in=e, Be=Be, uu=uu, vv=vv, sum=total, sum_tol=tol, iu=iu, iv=iv, bu=bu, bv=bv)


def keep_masks(d):
    """(keep_u, keep_v) [N,H,W] bool: False on the ring and where a kink rule leaves the pixel out (maxima per item); and the
    excluded share of the interior (the larger of the two)."""
    e, uu, vv = np.abs(d["e_in"]), np.abs(d["uu"]), np.abs(d["vv"])
    mx = lambda a: a.max(axis=(1, 2), keepdims=True)  # noqa: E731
    no_e = e < KINK * mx(e)
    no_u = (uu > 0) & (uu < KINK * mx(uu))
    no_v = (vv > 0) & (vv < KINK * mx(vv))
    N, h, w = e.shape
    ku, kv = np.zeros((N, h + 2, w + 2), bool), np.zeros((N, h + 2, w + 2), bool)
    ku[:, 1:-1, 1:-1], kv[:, 1:-1, 1:-1] = ~(no_e | no_u), ~(no_e | no_v)
    share = max(float((no_e | no_u).mean()), float((no_e | no_v).mean()))
    return ku, kv, share


def prefill(N, H, W, scale):
    """A NaN-free sentinel for a gradient plane, of the size of the reference's largest increment (`scale`): +-(1 .. 7) / 7 of
    it, so that the increment stays visible beside what the plane holds (the data term's gradient is of that order at the
    reference's CN_max; with l2 and a short step the increment is far smaller, and a fixed prefill would swallow it)."""
    idx = np.arange(N * H * W).reshape(N, H, W)
    return r32((1.0 + idx % 7) / 7.0 * np.where(idx % 2 == 0, 1.0, -1.0) * scale)

"""Case tables, f64 references, derived bounds, comparison functions and mutants for the simulation-side kernels of csrc/loss.hip
and csrc/rollout.hip: the advection-diffusion step and its CFL time step (mc_adnet_step, inherited by mc_rollout_*), the three
network-input builders, the roll-forward update, the wall condition and the on-device batch assembly
(tests/test_hip_step_kernels.py on the GPU, tests/test_step_cases_host.py on the CPU).

Inputs are rounded to f32 first (`r32`), so the reference sees what the kernel reads.  U = 2^-24 is the unit roundoff of f32; the
library is built with -ffp-contract=off, so every operation rounds once and the counts below are literal.

The step.  r = Tc + dt (-uu dTdx - vv dTdy + lap + q),  uu = s u,  dTdx = gl [uu > 0] + gr [uu < 0],  gl = (Tc - Tl) / dxl,
lap = (gr - gl) / (0.5 dxr + 0.5 dxl) + (gb - gt) / (0.5 dyb + 0.5 dyt).  The longest chain runs through the Laplacian:

  K_STEP = 10  Tc - Tl (1), / dxl (2), gr - gl (3), the denominator's sum (4; its two halvings are exact), the division (5),
               lap_x + lap_y (6), the sum of the bracket: (adv_x - adv_y) + lap (7), + q (8), x dt (9), Tc + (10).  The advective
               chain is shorter: s u (1), the gradient (2, 3), the product (4), the difference of the two (5), then 7 .. 10.

The per-pixel bound on the increment T_next - T_prev is U (K_STEP M + E).  M is the reference's expression with every difference
replaced by the sum of the absolute values, |Tc| included for the final add:
  M = |Tc| + dt (|uu| Gx + |vv| Gy + (Gr + Gl) / denx + (Gb + Gt) / deny + |q|),  Gl = (|Tc| + |Tl|) / dxl, Gx the upwind one.
E carries the coordinate differences.  x0 - xm with xm >= x0 / 2 is exact in f32 by Sterbenz's lemma, and so is every
difference against the wall coordinate 0 (x - 0); this covers the whole uniform grid right of its second column.  The others --
4 - x with x < 2, 1 - y with y < 0.5, and a stretched spacing that more than doubles its coordinate -- round once, relative to the
spacing itself: a gradient divided by such a spacing and the Laplacian's denominator built from it carry one more U each,
  E = dt (|uu| e_up Gx + |vv| e_up Gy + ((e_r Gr + e_l Gl) + max(e_l, e_r) (Gr + Gl)) / denx + the same in y),  e in {0, 1}.

The CFL step is compared bit for bit with a numpy evaluation in np.float32 (f32 division is correctly rounded on both sides:
tests/test_hip_rollout.py::test_cfl_step_is_per_member already relies on it) and within 4 U relative of the same expression in
f64: s u (1), the spacing (1), x 0.5 cn (1; 0.5 cn itself is exact), the division (1).

The viscosity channel log10(clip(exp(-ln FKT T + ln FKP (1 - y)), 1e-8, 1)) / 8.  E_ETA of tests/loss_cases.py (imported, not
derived twice) is the relative error of eta in units of U, under the conditions stated there (logf and expf 1 ulp).  The
channel's absolute bound is -log1p(-E_ETA U) / (8 ln 10) plus log10f's own error on the result, ULP_LOG10 ulp of |log10 eta| / 8;
the factor 0.125 is exact.  The ROCm installation carries no accuracy table of the device math library, so ULP_LOG10 = 2 is a
CONDITION, as the 1 ulp of logf / expf is.  A pixel clipped in both evaluations equals -1 or 0 exactly.

The velocity scale s = 5 exp(1.80167667 RaQ/10 + 0.4330392 ln FKT - 0.46052953 ln FKP).  The kernel's three constants are f32
(U each, relative); a1 = RaQ x 0.1f x 1.80167667f carries two constants and two products (4 U |a1|), a2 and a3 logf's 2 U, one
constant and one product (4 U each), the two additions 2 U A with A = |a1| + |a2| + |a3|: the argument is off by at most 6 U A;
expf adds 2 U and the product with 5 one more: K_SCALER_ARG = 6, K_SCALER_OUT = 3.  1 / s and everything multiplied by it are
checked bit for bit against the KERNEL's s, so the targets stay bit-checkable."""
import functools
import math
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
import loss_cases as Lc  # noqa: E402
from loss_cases import PARAS3, U, r32, stored  # noqa: E402,F401

f64 = torch.float64
F32 = np.float32
K_STEP = 10
K_DT = 4
K_SCALER_ARG, K_SCALER_OUT = 6, 3
ULP_LOG10 = 2                      # a condition (see the module docstring)
CN = 0.1
VEL_AMP, VEL_AMP_FINE = 100.0, 1000.0   # smooth_field (amplitude 0.1) x this.  At the CFL step the advective increment does not
FINE = 100000                           # depend on it and the diffusive one falls with it: a grid of more pixels than FINE needs more
BALANCE = 100.0                    # the largest advective and diffusive increments of a case lie within this factor

# [n, H, W]; see the issue's table
STEP_SHAPES = [(1, 3, 3), (2, 4, 5), (3, 5, 6), (2, 9, 70), (4, 33, 130)]
STEP_BIG = (1, 513, 520)           # the only shape whose 1024-block grid strides
BUILD_SHAPES = [(1, 1, 1), (3, 5, 6), (2, 33, 130)]
BUILD_BIG = (1, 513, 520)
WALL_SHAPES = [(1, 2, 3), (3, 5, 6), (2, 33, 130)]
ASM_SHAPES = [(1, 1), (5, 6), (33, 130)]
ASM_M = 5
ASM_PAIRS = [(4, 3), (0, 1), (4, 3), (1, 0), (2, 4)]          # the last item, an item twice, an order reversed
ASM_IDX = [4, 0, 4, 3, 1, 0]


# ---- grids ----------------------------------------------------------------------------------------------------------------
def grid_uniform(H, W):
    """The grid of tests/test_hip_rollout.py: cell centres, walls stored as 0 / 4 and 0 / 1."""
    xs = np.concatenate(([0.0], (np.arange(W - 2) + 0.5) * 4.0 / (W - 2), [4.0])) if W > 1 else np.array([2.0])
    ys = np.concatenate(([0.0], (np.arange(H - 2) + 0.5) * 1.0 / (H - 2), [1.0])) if H > 1 else np.array([0.5])
    return (np.broadcast_to(xs[None, :], (H, W)).astype(F32).copy(), np.broadcast_to(ys[:, None], (H, W)).astype(F32).copy())


def _spacings(n):
    """n spacings: small towards both ends, and alternately 0.7 and 1.3 of that, so that neighbours differ by far more than 20 %."""
    k = np.arange(n)
    return (1.0 + 0.5 * np.sin(np.pi * (k + 0.5) / n)) * np.where(k % 2 == 0, 0.7, 1.3)


def _axis(n, length):
    if n == 1:
        return np.array([0.5 * length]), 0.0
    s = _spacings(n - 1)
    s = s * (length / s.sum())
    a = np.concatenate(([0.0], np.cumsum(s)))
    a[-1] = length
    return a, float(s.min())


def grid_stretched(H, W, finite_walls=False):
    """Stretched and sheared: xc clustered towards both side walls and shifted by a row-dependent amount, yc clustered towards top
    and bottom and shifted by a column-dependent amount.  The stored wall entries are NaN (the step kernels must substitute 0 / 4
    and 0 / 1 and never read them) unless `finite_walls` (for the kernels that read yc everywhere)."""
    X, sx = _axis(W, 4.0)
    Y, sy = _axis(H, 1.0)
    xc = np.broadcast_to(X[None, :], (H, W)).copy()
    yc = np.broadcast_to(Y[:, None], (H, W)).copy()
    xc[:, 1:-1] += (0.15 * sx * np.sin(1.7 * np.arange(H) + 0.3))[:, None]
    yc[1:-1, :] += (0.15 * sy * np.cos(2.3 * np.arange(W) + 0.1))[None, :]
    if not finite_walls:
        if W > 1:
            xc[:, 0] = xc[:, -1] = np.nan
        if H > 1:
            yc[0, :] = yc[-1, :] = np.nan
    return xc.astype(F32), yc.astype(F32)


def with_walls(xc, yc):
    """f64 copies with the wall coordinates 0 / 4 and 0 / 1 written in, as the reference does to its inputs."""
    x, y = np.asarray(xc, np.float64).copy(), np.asarray(yc, np.float64).copy()
    x[:, 0], x[:, -1] = 0.0, 4.0
    y[0, :], y[-1, :] = 0.0, 1.0
    return x, y


# ---- the advection-diffusion step -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(N, H, W, stretched):
    """Members with different fields, vel_scale and RaQ.  An interior pixel with u == 0 and another with v == 0 in every member
    (one interior pixel: u == 0 only); with N >= 2 the LAST member is at rest.  f64 arrays holding f32 values."""
    seed = 1000 * N + 7 * H + W + (500 if stretched else 0)
    amp = VEL_AMP_FINE if H * W > FINE else VEL_AMP
    u = fields.smooth_field(N, H, W, seed + 1) * amp
    v = fields.smooth_field(N, H, W, seed + 2) * amp
    u[:, 1, 1] = 0.0
    if (H - 2) * (W - 2) > 1:
        v[:, H - 2, W - 2] = 0.0
    if N >= 2:
        u[N - 1] = 0.0
        v[N - 1] = 0.0
    xc, yc = grid_stretched(H, W) if stretched else grid_uniform(H, W)
    T = fields.temperature_field(N, H, W, seed + 3)
    T[:, 1:-1, :] += 0.05 * fields.smooth_field(N, H, W, seed + 5, amp=1.0)[:, 1:-1, :]      # (a 3-wide plume field is flat along x)
    T = np.clip(T, 0.0, 1.35).astype(F32).astype(np.float64)
    c = dict(N=N, H=H, W=W, stretched=stretched, xc=xc, yc=yc,
             u=u.astype(F32).astype(np.float64), v=v.astype(F32).astype(np.float64),
             T=T,
             raq_field=(2.5 + 5.0 * fields.smooth_field(N, H, W, seed + 4)).astype(F32).astype(np.float64),
             raq=np.array([1.5, 2.5, 4.0, 9.0])[:N].astype(F32).astype(np.float64),
             vs=np.array([0.5, 1.7, 3.0, 0.9])[:N].astype(F32).astype(np.float64))
    return c


def _inexact(a, b):
    """1.0 where the f32 difference a - b (a >= b >= 0) is not exact by Sterbenz's lemma or by b == 0."""
    return ((b != 0.0) & (b < 0.5 * a)).astype(np.float64)


def step64(c, dt, s=None, raq=None, mag=False, **mut):
    """oracle.ref_cpu.adnet_step restated by index, with dt given, a per-member velocity scale s [N] (None = 1) and RaQ as a field
    [N, H, W] or per member [N]: T_next [N, H, W].  mag = True: (M, E) of the module docstring on the interior.  Mutants (`mut`):
    no_heat, heat_075, central, swap_upwind, gr_by_dxl, uniform_lap, grid_row0, stored_walls, side_col0, scale_u_only."""
    N, H, W = c["N"], c["H"], c["W"]
    T, dt = c["T"], float(dt)
    raq = c["raq"] if raq is None else raq
    if mut.get("stored_walls"):
        x, y = np.asarray(c["xc"], np.float64), np.asarray(c["yc"], np.float64)
    else:
        x, y = with_walls(c["xc"], c["yc"])
    if mut.get("grid_row0"):
        x, y = np.broadcast_to(x[0:1, :], (H, W)), np.broadcast_to(y[:, 0:1], (H, W))
    In = (slice(None), slice(1, -1), slice(1, -1))
    sv = np.ones(N) if s is None else np.asarray(s, np.float64)
    uu = sv[:, None, None] * c["u"][In]
    vv = (np.ones(N) if mut.get("scale_u_only") else sv)[:, None, None] * c["v"][In]
    q = raq[In] if raq.ndim == 3 else raq[:, None, None] * np.ones((1, H - 2, W - 2))
    x0, xm, xp = x[1:-1, 1:-1], x[1:-1, :-2], x[1:-1, 2:]
    y0, ym, yp = y[1:-1, 1:-1], y[:-2, 1:-1], y[2:, 1:-1]
    dxl, dxr, dyt, dyb = x0 - xm, xp - x0, y0 - ym, yp - y0
    Tc, Tl, Tr, Tt, Tb = T[In], T[:, 1:-1, :-2], T[:, 1:-1, 2:], T[:, :-2, 1:-1], T[:, 2:, 1:-1]
    denx, deny = 0.5 * dxr + 0.5 * dxl, 0.5 * dyb + 0.5 * dyt
    if mut.get("uniform_lap"):
        denx, deny = 4.0 / (W - 2) + 0.0 * denx, 1.0 / (H - 2) + 0.0 * deny
    if mag:
        a = np.abs
        Gl, Gr, Gt, Gb = (a(Tc) + a(Tl)) / dxl, (a(Tr) + a(Tc)) / dxr, (a(Tc) + a(Tt)) / dyt, (a(Tb) + a(Tc)) / dyb
        el, er, et, eb = _inexact(x0, xm), _inexact(xp, x0), _inexact(y0, ym), _inexact(yp, y0)
        Gx, ex = Gl * (uu > 0) + Gr * (uu < 0), el * (uu > 0) + er * (uu < 0)
        Gy, ey = Gt * (vv > 0) + Gb * (vv < 0), et * (vv > 0) + eb * (vv < 0)
        M = a(Tc) + dt * (a(uu) * Gx + a(vv) * Gy + (Gr + Gl) / denx + (Gb + Gt) / deny + a(q))
        E = dt * (a(uu) * ex * Gx + a(vv) * ey * Gy + ((er * Gr + el * Gl) + np.maximum(el, er) * (Gr + Gl)) / denx
                  + ((eb * Gb + et * Gt) + np.maximum(et, eb) * (Gb + Gt)) / deny)
        return M, E
    gl, gr, gt, gb = (Tc - Tl) / dxl, (Tr - Tc) / (dxl if mut.get("gr_by_dxl") else dxr), (Tc - Tt) / dyt, (Tb - Tc) / dyb
    if mut.get("central"):
        dTdx, dTdy = 0.5 * (gl + gr) * (uu != 0), 0.5 * (gt + gb) * (vv != 0)
    elif mut.get("swap_upwind"):
        dTdx, dTdy = gr * (uu > 0) + gl * (uu < 0), gb * (vv > 0) + gt * (vv < 0)
    else:
        dTdx, dTdy = gl * (uu > 0) + gr * (uu < 0), gt * (vv > 0) + gb * (vv < 0)
    lap = (gr - gl) / denx + (gb - gt) / deny
    heat = 0.0 if mut.get("no_heat") else (0.75 * q if mut.get("heat_075") else q)
    Tn = np.empty_like(T)
    Tn[In] = Tc + dt * (-uu * dTdx - vv * dTdy + lap + heat)
    Tn[:, :, 0], Tn[:, :, -1] = Tn[:, :, 1], Tn[:, :, -2]
    if mut.get("side_col0"):
        Tn[:, :, 0], Tn[:, :, -1] = T[:, :, 0], T[:, :, -1]
    Tn[:, 0, :], Tn[:, -1, :] = 1.0, 0.0
    return Tn


def increments(c, dt, s=None, raq=None):
    """(largest advective, largest diffusive increment) of a step, over the members that move."""
    no_v = dict(c, u=0.0 * c["u"], v=0.0 * c["v"])
    z = np.zeros(c["N"])
    diff = step64(no_v, dt, None, z) - c["T"]
    adv = (step64(c, dt, s, z) - c["T"]) - diff
    In = (slice(None), slice(1, -1), slice(1, -1))
    return float(np.abs(adv[In]).max()), float(np.abs(diff[In]).max())


def dt32(c, s=None, cn=CN, members=None, row1_only=False):
    """The header's expression min(0.5 cn dx / uv, 0.5 dx2 dx2 / (dx2 + dx2)) evaluated operation by operation in np.float32."""
    m = list(range(c["N"])) if members is None else members
    x = np.asarray(c["xc"], F32).copy()
    x[:, 0], x[:, -1] = F32(0.0), F32(4.0)
    d = x[1:-1, 1:-1] - x[1:-1, :-2]
    dx = (d[:1] if row1_only else d).min()
    sv = np.ones(len(m), F32) if s is None else np.asarray(s, F32)[m]
    su = sv[:, None, None] * c["u"][m].astype(F32)[:, 1:-1, 1:-1]
    sw = sv[:, None, None] * c["v"][m].astype(F32)[:, 1:-1, 1:-1]
    uv = max(np.abs(su).max(), np.abs(sw).max())
    assert d.dtype == F32 and su.dtype == F32 and uv.dtype == F32
    with np.errstate(divide="ignore"):
        adv = F32(0.5) * F32(cn) * dx / uv
    dx2 = dx * dx
    dif = F32(0.5) * (dx2 * dx2) / (dx2 + dx2)
    out = min(adv, dif)
    assert out.dtype == F32
    return out


def dt64(c, s=None, cn=CN, members=None):
    m = list(range(c["N"])) if members is None else members
    x, _ = with_walls(c["xc"], c["yc"])
    dx = float((x[1:-1, 1:-1] - x[1:-1, :-2]).min())
    sv = np.ones(len(m)) if s is None else np.asarray(s, np.float64)[m]
    uv = float(max(np.abs(sv[:, None, None] * c["u"][m][:, 1:-1, 1:-1]).max(), np.abs(sv[:, None, None] * c["v"][m][:, 1:-1, 1:-1]).max()))
    cn = float(F32(cn))
    return min(0.5 * cn * dx / uv if uv > 0 else math.inf, 0.25 * dx * dx)


def check_dt(got, c, s=None, members=None):
    """Failures of a CFL step against the f32 evaluation (bits) and the f64 one (K_DT U relative)."""
    out = []
    want = dt32(c, s, members=members)
    if not (np.isfinite(got) and F32(got).tobytes() == want.tobytes()):
        out.append(f"dt {float(got)!r} is not the f32 evaluation {float(want)!r}")
    ref = dt64(c, s, members=members)
    if not abs(float(got) - ref) <= K_DT * U * ref:
        out.append(f"dt {float(got)!r} against f64 {ref!r}: {abs(float(got) - ref) / (U * ref):.2f} U")
    return out, abs(float(got) - ref) / (K_DT * U * ref)


def check_step(c, got, dt, s=None, raq=None):
    """T_next [N, H, W] (an f64 tensor or array holding what the kernel stored) against step64 with the same dt: the increment on
    the interior within U (K_STEP M + E), wall rows exactly 1 / 0, side columns bit-equal to their neighbours.
    Returns (failures, worst err / tol)."""
    got = np.asarray(got, np.float64)
    ref = step64(c, dt, s, raq)
    M, E = step64(c, dt, s, raq, mag=True)
    In = (slice(None), slice(1, -1), slice(1, -1))
    tol = U * (K_STEP * M + E)
    worst, bad = Lc.compare(torch.from_numpy(got[In] - c["T"][In]), torch.from_numpy(ref[In] - c["T"][In]), torch.from_numpy(tol))
    out = []
    if bool(bad.any()):
        out.append(f"increment: {int(bad.sum())} interior pixels beyond the bound, worst err / tol {worst:.3g}")
    if not ((got[:, 0, :] == 1.0).all() and (got[:, -1, :] == 0.0).all()):
        out.append("a wall row is not exactly 1 / 0")
    g32 = got.astype(F32)
    if not (np.array_equal(g32[:, 1:-1, 0].view(np.int32), g32[:, 1:-1, 1].view(np.int32))
            and np.array_equal(g32[:, 1:-1, -1].view(np.int32), g32[:, 1:-1, -2].view(np.int32))):
        out.append("a side column is not a copy of its neighbour")
    return out, worst


# ---- the viscosity channel and the velocity scale -------------------------------------------------------------------------
def visc64(T, y, paras, lo=Lc.ETA_LO):
    """(V, tol, exact): the channel in f64, its absolute bound, and the pixels clipped in both evaluations (V is -1 or 0 there).
    T [N, H, W], y [H, W] or [N, H, W], paras [N, 3]: f64 tensors."""
    eta, _, e = Lc.eta_error(T, y, paras)
    if lo != Lc.ETA_LO:
        eta = torch.clip(torch.exp(Lc.eta64(T, y, paras)[1]), lo, 1.0)
    lg = torch.log10(eta)
    tol = -torch.log1p(-e * U) / (8.0 * math.log(10.0)) + ULP_LOG10 * 2.0 * U * lg.abs() / 8.0
    exact = (e == 0) & ((eta == 1.0) | (eta == Lc.ETA_LO))
    V = torch.where(exact, torch.round(lg / 8.0), lg / 8.0)            # log10(f32(1e-8)) / 8 is -1 to 3e-10: the kernel's is -1
    return V, torch.where(exact, torch.zeros_like(tol), tol), exact


def scaler64(paras):
    """(s, tol): 5 exp(1.80167667 RaQ/10 + 0.4330392 ln FKT - 0.46052953 ln FKP) of paras [N, 3] in f64 and its bound."""
    a1, a2, a3 = paras[:, 0] / 10.0 * 1.80167667, torch.log(paras[:, 1]) * 0.4330392, torch.log(paras[:, 2]) * -0.46052953
    s = 5.0 * torch.exp(a1 + a2 + a3)
    A = a1.abs() + a2.abs() + a3.abs()
    return s, s * (torch.expm1(K_SCALER_ARG * U * A) * (1.0 + K_SCALER_OUT * U) + K_SCALER_OUT * U)


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def f32op(fn, *a):
    """One f32 operation in numpy on f32 copies of the operands: what a single-rounding kernel expression must give, bit for bit."""
    out = fn(*[np.asarray(x, np.float64).astype(F32) for x in a])
    assert out.dtype == F32
    return t64(out)


def bcast(vals, H, W):
    """[N] -> [N, H, W]."""
    return t64(vals).view(-1, 1, 1).expand(-1, H, W).clone()


def plant_seams(T, y, paras):
    """Two pixels of member 0 moved onto the two seams of the clip (arg = ln 1e-8 and arg = 0), as near as an f32 T gets: within
    E_ETA of each; and the top quarter of member 0 cooled to 2 % of itself, so that the member whose parameters clip at 1e-8 in
    its hot part clips at 1 there, whatever the other members are.  In place; cases of fewer than four pixels are left alone."""
    H, W = T.shape[-2:]
    if H * W < 4:
        return T
    T[0, (3 * H + 3) // 4:] *= 0.02
    T[0] = r32(T[0])
    lt, lp = math.log(float(paras[0, 1])), math.log(float(paras[0, 2]))
    for k, seam in enumerate((math.log(Lc.ETA_LO), 0.0)):
        i, j = divmod(1 + k, W)
        T[0, i, j] = r32((lp * (1.0 - float(y[i, j])) - seam) / lt)
    return T


# ---- the input builders, the roll-forward update, the wall condition ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build_case(N, H, W):
    """T, dt, u_prev, v_prev [N, H, W]; xc, yc: the stretched grid with finite walls; ycc: the uniform depth, which differs."""
    seed = 2000 + 100 * N + H
    xc, yc = grid_stretched(H, W, finite_walls=True)
    ycc = grid_uniform(H, W)[1]
    rng = np.random.RandomState(seed)
    paras = r32(PARAS3[np.arange(N) % 3])
    field = lambda k: r32(fields.temperature_field(N, H, W, seed + k) if H > 1 else rng.uniform(0, 1.3, (N, H, W)))  # noqa: E731
    return dict(N=N, H=H, W=W, T=plant_seams(field(1), t64(ycc), paras), Tn=plant_seams(field(7), t64(yc), paras),
                xc=t64(xc), yc=t64(yc), ycc=t64(ycc), paras=paras, nd=r32(rng.uniform(0, 1, (N, 3))),
                dt=r32(1e-4 * (1.0 + fields.smooth_field(N, H, W, seed + 2))), up=r32(fields.smooth_field(N, H, W, seed + 3)),
                vp=r32(fields.smooth_field(N, H, W, seed + 4)), u=r32(fields.smooth_field(N, H, W, seed + 5)),
                v=r32(fields.smooth_field(N, H, W, seed + 6)))


def build_input_ref(c, unet, depth="ycc", lo=Lc.ETA_LO, quarter=False):
    """[(name, ref [N, H, W], tol [N, H, W])] of mc_ts_build_input (unet False) or mc_ts_build_input_unet; tol 0 = bit for bit.
    depth = 'yc', quarter (the depth / 4) and lo = 1e-7 are mutants."""
    N, H, W = c["N"], c["H"], c["W"]
    y = c[depth] * (0.25 if quarter else 1.0)
    V, vt, _ = visc64(c["T"], y, c["paras"], lo)
    z = torch.zeros((N, H, W), dtype=f64)
    ex = lambda t: (t.expand(N, H, W).clone(), z)  # noqa: E731
    xq, yq = f32op(lambda a: a * F32(0.25), c["xc"]), f32op(lambda a: a * F32(0.25), c["yc"])
    nd = [ex(c["nd"][:, k].view(-1, 1, 1)) for k in range(3)]
    if unet:
        chans = [ex(xq), ex(yq), ex(c["dt"]), *nd, (V, vt), ex(c["T"]), ex(c["up"]), ex(c["vp"])]
        names = ("xc/4", "yc/4", "dt", "nd0", "nd1", "nd2", "V", "T", "u_prev", "v_prev")
    else:
        chans = [ex(xq), ex(yq), (V, vt), *nd, ex(c["T"])]
        names = ("xc/4", "yc/4", "V", "nd0", "nd1", "nd2", "T")
    return [(n, r, t) for n, (r, t) in zip(names, chans)]


def roll_x0(c, C):
    """The batch tensor x [N, C, H, W] before the update: raw xc, yc (unscaled), dt, the parameters, and old V, T, u, v[, more]."""
    N, H, W = c["N"], c["H"], c["W"]
    g = torch.Generator().manual_seed(17 * H + C)
    x = r32(torch.randn((N, C, H, W), generator=g, dtype=f64))
    x[:, 0], x[:, 1] = c["xc"], c["yc"]
    return x


def roll_forward_ref(c, x0, update_v, depth=None, quarter=False, lo=Lc.ETA_LO):
    """(ref [N, C, H, W], tol): channels 7, 8, 9 = Tn, u, v; channel 6 = the viscosity of Tn at the depth of x0's channel 1 when
    update_v, else untouched; everything else untouched.  depth = 'ycc' and quarter are mutants."""
    ref, tol = x0.clone(), torch.zeros_like(x0)
    if update_v:
        y = x0[:, 1] if depth is None else c[depth].expand_as(x0[:, 1])
        ref[:, 6], tol[:, 6], _ = visc64(c["Tn"], y * (0.25 if quarter else 1.0), c["paras"], lo)
    ref[:, 7], ref[:, 8], ref[:, 9] = c["Tn"], c["u"], c["v"]
    return ref, tol


def wall_case(N, H, W):
    """(input with NaN in its own wall rows and side columns, expected output)."""
    src = r32(fields.smooth_field(N, H, W, 3000 + H, amp=1.0) + 0.5)
    ref = src.clone()
    ref[:, :, 0], ref[:, :, -1] = src[:, :, 1], src[:, :, W - 2]
    ref[:, 0, :], ref[:, -1, :] = 1.0, 0.0
    src = src.clone()
    src[:, :, 0] = src[:, :, -1] = float("nan")
    src[:, 0, :] = src[:, -1, :] = float("nan")
    return src, ref


def check_channels(chans, got):
    """`chans` of build_input_ref against got [N, C, H, W]: (failures, worst err / tol of the toleranced channels)."""
    names = [n for n, _, _ in chans]
    return Lc.check_planes(names, [got[:, k] for k in range(len(chans))], [r for _, r, _ in chans], [t for _, _, t in chans])


# ---- the assemblers ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store_case(H, W, cy):
    """A store of ASM_M items: T [m, H, W], uv [m, cy, H, W] (the GPU test overwrites the planes ADTime must skip with NaN), t,
    paras, paras_nd, xc, yc (stretched, finite walls) and a second depth ycc that is nobody's."""
    m, seed = ASM_M, 4000 + 10 * H + cy
    xc, yc = grid_stretched(H, W, finite_walls=True)
    rng = np.random.RandomState(seed)
    T = r32(fields.temperature_field(m, H, W, seed + 1) if H > 1 else rng.uniform(0, 1.3, (m, H, W)))
    uv = r32(np.stack([fields.smooth_field(m, H, W, seed + 2 + k, amp=30.0) for k in range(cy)], 1))
    paras = PARAS3[np.arange(m) % 3].copy()
    paras[3:, 0] += 1.25                                                     # items 3, 4: other scalers than items 0, 1
    T = plant_seams(T, t64(yc), r32(paras))
    return dict(m=m, H=H, W=W, cy=cy, T=T, uv=uv, t=r32(np.cumsum(rng.uniform(1e-5, 1e-3, m))), paras=r32(paras),
                nd=r32(rng.uniform(0, 1, (m, 3))), xc=t64(xc), yc=t64(yc), ycc=t64(grid_uniform(H, W)[1]))


def _item_common(S, i0, s_kernel, depth, quarter, lo, by_s):
    H, W = S["H"], S["W"]
    s64, s_tol = scaler64(S["paras"][i0:i0 + 1])
    s_k = float(s64[0]) if s_kernel is None else float(s_kernel)             # (host tests: the f64 scale stands in for the kernel's)
    inv = F32(s_k) if by_s else F32(1.0) / F32(s_k)
    V, vt, _ = visc64(S["T"][i0:i0 + 1], S[depth] * (0.25 if quarter else 1.0), S["paras"][i0:i0 + 1], lo)
    z = torch.zeros((H, W), dtype=f64)
    nd = [(S["nd"][i0, k].expand(H, W).clone(), z) for k in range(3)]
    return s64[0], s_tol[0], inv, (V[0], vt[0]), z, nd


def adtime_item_ref(S, i0, i1, s_kernel=None, depth="yc", quarter=False, lo=Lc.ETA_LO, by_s=False):
    """One slot of mc_assemble_adtime_batch from its item pair alone: (x channels, y channels, s, s_tol, paras) with
    channels = [(name, ref [H, W], tol)]."""
    H, W = S["H"], S["W"]
    s, s_tol, inv, V, z, nd = _item_common(S, i0, s_kernel, depth, quarter, lo, by_s)
    mul = lambda a: f32op(lambda p: p * inv, a)  # noqa: E731
    dt = f32op(lambda a, b: a - b, S["t"][i1], S["t"][i0]).expand(H, W).clone()
    x = [("xc", S["xc"], z), ("yc", S["yc"], z), ("t1-t0", dt, z), ("nd0", *nd[0]), ("nd1", *nd[1]), ("nd2", *nd[2]), ("V", *V),
         ("T", S["T"][i0], z), ("u/s", mul(S["uv"][i0, 0]), z), ("v/s", mul(S["uv"][i0, 1]), z)]
    y = [("u1/s", mul(S["uv"][i1, 0]), z), ("v1/s", mul(S["uv"][i1, 1]), z), ("T1", S["T"][i1], z)]
    return x, y, s, s_tol, S["paras"][i0]


def newad_item_ref(S, i0, s_kernel=None, depth="yc", quarter=False, lo=Lc.ETA_LO, by_s=False):
    """One slot of mc_assemble_newad_batch: (x channels, y channels, s, s_tol, t_weight)."""
    s, s_tol, inv, V, z, nd = _item_common(S, i0, s_kernel, depth, quarter, lo, by_s)
    mul = lambda a: f32op(lambda p: p * inv, a)  # noqa: E731
    q = lambda a: f32op(lambda p: p * F32(0.25), a)  # noqa: E731
    x = [("xc/4", q(S["xc"]), z), ("yc/4", q(S["yc"]), z), ("V", *V), ("nd0", *nd[0]), ("nd1", *nd[1]), ("nd2", *nd[2]),
         ("T", S["T"][i0], z)]
    y = [("u/s", mul(S["uv"][i0, 0]), z), ("v/s", mul(S["uv"][i0, 1]), z)]
    if S["cy"] > 2:
        y.append(("p", S["uv"][i0, 2], z))
    return x, y, s, s_tol, S["t"][i0]


def check_item(chans, got):
    """Channels [(name, ref [H, W], tol)] against got [C, H, W]."""
    return Lc.check_planes([n for n, _, _ in chans], [got[k] for k in range(len(chans))], [r for _, r, _ in chans],
                           [t for _, _, t in chans])


def as_got(chans):
    """A reference's channels as a kernel would have stored them."""
    return torch.stack([stored(r) for _, r, _ in chans])


def clip_shares(T, y, paras):
    """(share clipped at 1e-8, share clipped at 1, pixels within E_ETA of the lower seam, of the upper seam) of a viscosity."""
    _, arg, A = Lc.eta64(T, y, paras)
    d = 5.0 * U * A + 2.0 * U
    lo = math.log(Lc.ETA_LO)
    return (float((arg < lo).double().mean()), float((arg > 0).double().mean()),
            int(((arg - lo).abs() <= d).sum()), int((arg.abs() <= d).sum()))

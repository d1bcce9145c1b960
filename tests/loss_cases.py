"""Case tables, f64 references, derived bounds, comparison functions and mutants for the Stokes loss kernels of csrc/loss.hip and
the curl head of csrc/curl_head.hip (tests/test_hip_loss_kernels.py on the GPU, tests/test_loss_cases_host.py on the CPU).

The references restate oracle/ref_cpu.py with `ra` and `inv_h` as parameters (the oracle fixes both); the host tests assert once
that the restatement equals the oracle at ra = 1, inv_h = 126.

Bounds.  U = 2^-24 is the unit roundoff of f32.  Every bound is (count of roundings on the longest chain of the kernel's
expression) x U x (the sum of the magnitudes of the expression's addends, from the f64 reference).  The sum of magnitudes is the
same expression with every difference replaced by the sum of the absolute values (`mag=True` below); for a gradient, which is
linear in the weighted signs S, it is the adjoint of that all-positive operator applied to |S|, which autograd delivers.  The
kernels are built with -ffp-contract=off, so every operation rounds once and the counts are literal:

  K_RES = 12   residual: s u (1), the difference (2), x ih (3), dVdx + dVdx (4), + the normal difference (5), x the face
               viscosity (6; its own sum is one more rounding, relative, counted as 7), the difference of the two faces (8),
               x ih (9), the sum of the three groups (10, 11), + ra T (12)
  K_ADJ = 12   adjoint: S - S (1), x ih (2), the face viscosity's sum (3), x it (4), the sum of the four cross faces (5-7),
               x 0.25 ih (8), the sum of the three groups (9, 10), x s (11); one in hand for 2 ih (12).  The accumulation into
               the gradient buffer rounds once more, relative to the stored value: + U (|g0| + |ref|)
  E_ETA        relative error of the viscosity exp(-ln(FKT) T + ln(FKP) (1 - y)) in units of U: logf is 1 ulp = 2 U, each
               product and 1 - y one U more, the sum one U of A = |ln(FKT) T| + |ln(FKP) (1 - y)|: the argument is off by at
               most 5 U A, and expf adds 1 ulp: 5 A + 2.  A pixel whose argument lies outside [ln 1e-8, 0] by more than that is
               clipped in both evaluations and carries no error.
  K_GRAD = 20  data / derivative / divergence gradient: the l2 data term is the longest chain (the difference 1, su x bw twice
               3 + 3, cdat 3, four products) and up to six additions collect the terms of a pixel
  K_KINK = 3   e = (ut' - ut) - (u' - u) and D = 0.5 (u+ - u-) + 0.5 (v+ - v-): three roundings each
  K_OUT = 12   one |term| of a sum (at most 6: the difference, su x bw 3, the product, the square), its division and the f32
               store; the f32 running sum of a thread adds (its number of pixels) x U
"""
import functools
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fields  # noqa: E402

f64 = torch.float64
U = 2.0 ** -24
K_RES, K_ADJ, K_GRAD, K_KINK, K_OUT = 12, 12, 20, 3, 12
MAX_SHARE = 0.05                             # of the pixels a kink rule may leave out of one comparison: a condition on the INPUTS
RA, INV_H = 2.5, 63.0                        # neither the oracle's 1 nor its 126
ETA_LO = float(np.float32(1e-8))

# tile sizes of csrc/loss.hip (rows x 64 pixels) and its launch formulas, restated
LT_TH, LF_TH, MR_TH, MA_TH, TW = 32, 8, 16, 8, 64
SHAPES = [(5, 5), (9, 66), (17, 65), (33, 129), (34, 64)]      # see the issue's table: minimum; every halo column across a seam;
B = 3                                                          # one row past 16; one row past 32 and two seams; exact tile width
MANY = (256, 33, 129)                                          # every loop kernel walks more than one tile per block


def cdiv(a, b):
    return -(-a // b)


def tiles(H, W, th):
    return cdiv(W, TW) * cdiv(H, th)


def loss_blocks(N, H, W):
    return max(1, min(cdiv(1024, N), cdiv(H * W, 256)))


def grid_loss(N, H, W):
    return min(loss_blocks(N, H, W), tiles(H, W, LT_TH))


def grid_residual(N, H, W):
    return min(2 * loss_blocks(N, H, W), tiles(H, W, MR_TH))


def grid_fused(N, H, W):
    return max(1, min(cdiv(2048, N), tiles(H, W, LF_TH)))


def adds_per_thread(N, H, W, th, grid):
    """Pixels one thread adds into its f32 running sums: th / 4 rows per tile, ceil(tiles / blocks) tiles."""
    return (th // 4) * cdiv(tiles(H, W, th), grid)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def r32(a):
    """Rounded to f32 first, so that the reference sees what the kernel reads."""
    return torch.as_tensor(np.asarray(a, np.float64).astype(np.float32).astype(np.float64))


PARAS3 = np.array([[5.0, 1.0e9, 3.0], [3.0, 1.0e3, 30.0], [7.0, 10.0, 50.0]])      # clips at 1e-8; neither; clips at 1 (FKP > FKT)


@functools.lru_cache(maxsize=None)
def inputs(N, H, W, seed=500, noise=0.01):
    """u, v, p, T predictions, the four truth planes, yc, paras, scaler: f64 tensors holding f32 values."""
    d = dict(u=r32(fields.smooth_field(N, H, W, seed + 1, noise=noise)), v=r32(fields.smooth_field(N, H, W, seed + 2, noise=noise)),
             p=r32(fields.smooth_field(N, H, W, seed + 3, amp=0.5)), T=r32(fields.temperature_field(N, H, W, seed + 4)))
    d["truth"] = torch.stack([r32(fields.smooth_field(N, H, W, seed + 5)), r32(fields.smooth_field(N, H, W, seed + 6)),
                              r32(fields.smooth_field(N, H, W, seed + 7, amp=0.5)), r32(fields.temperature_field(N, H, W, seed + 8))], 1)
    d["yc"] = r32(np.broadcast_to(np.linspace(0, 1, H)[:, None], (H, W)).copy())
    rng = np.random.RandomState(seed + 9)
    d["paras"] = r32(PARAS3[np.arange(N) % 3])
    d["scaler"] = r32(30.0 + 50.0 * rng.uniform(size=N))                  # different per sample
    return d


# ---- momentum residual ----------------------------------------------------------------------------------------------------
def eta64(T, yc, paras):
    lt, lp = torch.log(paras[:, 1]).view(-1, 1, 1), torch.log(paras[:, 2]).view(-1, 1, 1)
    arg = -lt * T + lp * (1.0 - yc)
    return torch.clip(torch.exp(arg), ETA_LO, 1.0), arg, (lt * T).abs() + (lp * (1.0 - yc)).abs()


def eta_error(T, yc, paras):
    """(eta, its relative bound, E_ETA per pixel in units of U: 0 where both evaluations clip)."""
    eta, arg, A = eta64(T, yc, paras)
    darg = 5.0 * U * A
    clipped = (arg - darg > 0.0) | (arg + darg + 2.0 * U < math.log(ETA_LO))
    e = torch.where(clipped, torch.zeros_like(A), 5.0 * A + 2.0)
    rel = torch.where(clipped, torch.full_like(A, U), torch.expm1(darg) * (1.0 + 2.0 * U) + 2.0 * U)
    return eta, rel, e


def residual64(u, v, p, T, eta, s, ra=RA, ih=INV_H, cross=1.0, face="mean", mag=False):
    """R_x, R_y [N, H-2, W-2] of oracle.ref_cpu.momentum_residual with eta given, ra and ih free.  mag = True: the sum of the
    magnitudes of the addends (pass |u|, |v|, |p|, |T|).  cross = 0 and face = 'node' are mutants."""
    sub = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    s = s.view(-1, 1, 1)
    Uu, V = u * s, v * s
    if face == "mean":
        exf, eyf = 0.5 * (eta[:, :, :-1] + eta[:, :, 1:]), 0.5 * (eta[:, :-1, :] + eta[:, 1:, :])
    else:
        exf, eyf = eta[:, :, :-1], eta[:, :-1, :]
    Fx = 2.0 * exf * sub(Uu[:, :, 1:], Uu[:, :, :-1]) * ih
    Fy = 2.0 * eyf * sub(V[:, 1:, :], V[:, :-1, :]) * ih
    dVdx = 0.5 * sub(V[:, :, 2:], V[:, :, :-2]) * ih
    Tyf = eyf[:, :, 1:-1] * (sub(Uu[:, 1:, 1:-1], Uu[:, :-1, 1:-1]) * ih + cross * 0.5 * (dVdx[:, :-1] + dVdx[:, 1:]))
    dUdy = 0.5 * sub(Uu[:, 2:, :], Uu[:, :-2, :]) * ih
    Txf = exf[:, 1:-1, :] * (sub(V[:, 1:-1, 1:], V[:, 1:-1, :-1]) * ih + cross * 0.5 * (dUdy[:, :, :-1] + dUdy[:, :, 1:]))
    dpdx = 0.5 * sub(p[:, 1:-1, 2:], p[:, 1:-1, :-2]) * ih
    dpdy = 0.5 * sub(p[:, 2:, 1:-1], p[:, :-2, 1:-1]) * ih
    Rx = sub(sub(Fx[:, 1:-1, 1:], Fx[:, 1:-1, :-1]) * ih + sub(Tyf[:, 1:, :], Tyf[:, :-1, :]) * ih, dpdx)
    Ry = sub(sub(Fy[:, 1:, 1:-1], Fy[:, :-1, 1:-1]) * ih + sub(Txf[:, :, 1:], Txf[:, :, :-1]) * ih, dpdy) + ra * T[:, 1:-1, 1:-1]
    return Rx, Ry


def pad_ring(t):
    """[N, H-2, W-2] -> [N, H, W] with a ring of zeros (False)."""
    if t.dtype == torch.bool:
        return F.pad(t.to(torch.uint8), (1, 1, 1, 1)) > 0
    return F.pad(t, (1, 1, 1, 1))


def c_mom32(lam, N, H, W):
    """lambda / (N (H-2) (W-2)) as the kernels form it in f32."""
    f = np.float32
    return float(f(lam) / (f(N) * f(H - 2) * f(W - 2)))


class Residual:
    """Part B: everything mc_momentum_residual writes, from f64."""

    def __init__(self, d, lam, ra=RA, ih=INV_H, p_null=False):
        u, v, T, s = d["u"], d["v"], d["T"], d["scaler"]
        p = torch.zeros_like(u) if p_null else d["p"]
        N, H, W = u.shape
        self.eta, self.eta_rel, e = eta_error(T, d["yc"], d["paras"])
        self.Rx, self.Ry = residual64(u, v, p, T, self.eta, s, ra, ih)
        mx, my = residual64(u.abs(), v.abs(), p.abs(), T.abs(), self.eta, s, abs(ra), ih, mag=True)
        e3 = F.max_pool2d(e.unsqueeze(1), 3, 1)[:, 0]                    # the faces of a pixel read eta of its 3 x 3 neighbours
        self.bx, self.by = U * (K_RES + e3) * mx, U * (K_RES + e3) * my
        self.c = c_mom32(lam, N, H, W)
        self.sx, self.sy = pad_ring(self.c * torch.sign(self.Rx)), pad_ring(self.c * torch.sign(self.Ry))
        self.keep_x, self.keep_y = pad_ring(self.Rx.abs() > self.bx), pad_ring(self.Ry.abs() > self.by)
        ring = torch.ones((N, H, W), dtype=torch.bool)
        ring[:, 1:-1, 1:-1] = False
        self.keep_x |= ring                                              # the ring itself is exact: 0
        self.keep_y |= ring
        self.sums = (float(self.Rx.abs().sum()), float(self.Ry.abs().sum()))
        adds = adds_per_thread(N, H, W, MR_TH, grid_residual(N, H, W))
        self.sums_tol = (float(self.bx.sum()) + adds * U * self.sums[0], float(self.by.sum()) + adds * U * self.sums[1])
        self.kink = pad_ring((self.Rx.abs() <= self.bx) | (self.Ry.abs() <= self.by))

    def share(self):
        """Largest share of the interior that one sign comparison leaves out."""
        return max(1.0 - float(self.keep_x.double().mean()), 1.0 - float(self.keep_y.double().mean()))

    def dilated(self):
        """Pixels whose 3 x 3 neighbourhood holds a kink: left out of the gradient comparison of part C."""
        return F.max_pool2d(self.kink.double().unsqueeze(1), 3, 1, 1)[:, 0] > 0


def adjoint64(sx, sy, eta, s, ra=RA, ih=INV_H, mag=False, **mut):
    """(gu, gv, gp, gT) = d/d(u, v, p, T) of sum(sx R_x + sy R_y) with eta held fixed: autograd of the linear residual."""
    z = [torch.zeros_like(sx, requires_grad=True) for _ in range(4)]
    Rx, Ry = residual64(z[0], z[1], z[2], z[3], eta, s, ra, ih, mag=mag, **mut)
    ((sx[:, 1:-1, 1:-1] * Rx).sum() + (sy[:, 1:-1, 1:-1] * Ry).sum()).backward()
    return [t.grad for t in z]


def adjoint_bound(sx, sy, eta, s, ra=RA, ih=INV_H, e=None):
    m = adjoint64(sx.abs(), sy.abs(), eta, s, abs(ra), ih, mag=True)
    k = K_ADJ if e is None else K_ADJ + F.max_pool2d(e.unsqueeze(1), 3, 1, 1)[:, 0]
    return [U * k * t for t in m]


@functools.lru_cache(maxsize=None)
def adjoint_case(N, H, W, seed=700):
    """Part A: random S (zero on the outermost ring), eta in (1e-8, 1], a known field g0 in the gradient planes."""
    g = torch.Generator().manual_seed(seed + 131 * H + W)
    sx, sy = (pad_ring(r32(torch.randn((N, H - 2, W - 2), generator=g, dtype=f64))) for _ in range(2))
    eta = r32(10.0 ** (-8.0 * torch.rand((N, H, W), generator=g, dtype=f64)))
    eta = torch.clip(eta, float(np.nextafter(np.float32(1e-8), np.float32(1))), 1.0)
    s = inputs(N, H, W)["scaler"]
    g0 = r32(torch.randn((N, 5, H, W), generator=g, dtype=f64))          # channels u, v, T, p and one that is nobody's
    ref = adjoint64(sx, sy, eta, s)                                      # (u, v, p, T)
    tol = [b + U * (g0[:, ch].abs() + r.abs()) for b, ch, r in zip(adjoint_bound(sx, sy, eta, s), (0, 1, 3, 2), ref)]
    return dict(sx=sx, sy=sy, eta=eta, s=s, g0=g0, ref=ref, tol=tol)


# ---- data, derivative and divergence terms --------------------------------------------------------------------------------
def _red(d, l2):
    return (d * d).mean() if l2 else d.abs().mean()


def loss_fn64(t, x, ls, l2, frame=2):
    plain = _red(t - x, l2)
    if not ls:
        return plain, plain
    s = torch.clip(1.0 / (torch.amax(t, (1, 2), keepdim=True) - torch.amin(t, (1, 2), keepdim=True)), 1.0, 10.0)
    w = torch.full_like(t, 11.0)
    w[:, frame:-frame, frame:-frame] = 1.0
    return _red((t - x) * s * w, l2), plain


def dy_top(f):
    return f[:, 1:-1, :] - f[:, :-2, :]            # e[i] = f[i+1] - f[i], i in [0, H-3]


def dx_left(f):
    return f[:, :, 1:-1] - f[:, :, :-2]


def divergence(u, v):
    return 0.5 * (u[:, 1:-1, 2:] - u[:, 1:-1, :-2]) + 0.5 * (v[:, 2:, 1:-1] - v[:, :-2, 1:-1])


def wall_sum(m, wall0=False):
    left = 0.0 if wall0 else m[:, :, 0].mean()     # (mutant: the weight asked for at x == 0, where there is no divergence)
    return left + m[:, :, -1].mean() + m[:, 0, :].mean() + m[:, -1, :].mean()


def stokes_terms64(u, v, p, T, truth, *, p_pred, loss_type, ls, ld, l2, has_T=True, frame=2, swap_norm=False, wall0=False):
    """get_loss of the Unet branch (has_T) or the FluidNet branch, restated: (data, derivative, mass) terms of the loss --
    their sum is the loss -- and the six reported values."""
    ut, vt = truth[:, 0], truth[:, 1]
    lu, tu = loss_fn64(ut, u, ls, l2, frame)
    lv, tv = loss_fn64(vt, v, ls, l2, frame)
    zero = torch.zeros((), dtype=f64)
    lp = lT = zero
    if p_pred:
        sc, pl = loss_fn64(truth[:, 2], p, ls, l2, frame)
        lp = pl if has_T else sc
    if has_T:
        lT = loss_fn64(truth[:, 3 if p_pred else 2], T, ls, l2, frame)[1]
    k = (3.0 if p_pred else 2.0) + (1.0 if has_T else 0.0)
    data = (lu + lv + lp + lT) / k
    deriv = zero
    if ld:
        eu, ev = 126.0 * (dy_top(ut) - dy_top(u)).abs(), 126.0 * (dx_left(vt) - dx_left(v)).abs()
        N, H, W = u.shape
        du, dv = eu.sum() / (N * (H - 2) * W), ev.sum() / (N * H * (W - 2))
        if swap_norm:
            du, dv = eu.sum() / (N * H * (W - 2)), ev.sum() / (N * (H - 2) * W)
        deriv = (du + dv) / k
        if not ls:
            tu, tv = lu + du, lv + dv                   # the reference's aliasing quirk
    m = divergence(u, v).abs()
    mass = m.mean() if loss_type == 1 else wall_sum(m, wall0) if loss_type == 2 else zero
    return (data, deriv, mass), [data + deriv + mass, tu, tv, lp, lT, m.mean()]


def _spread(H, W, N, build):
    """d/da of build(a) at a leaf of ones: how an all-positive linear form spreads its weights over the pixels."""
    a = torch.ones((N, H, W), dtype=f64, requires_grad=True)
    b = torch.ones((N, H, W), dtype=f64, requires_grad=True)
    out = build(a, b)
    if not out.requires_grad:
        return torch.zeros((N, H, W), dtype=f64), torch.zeros((N, H, W), dtype=f64)
    ga, gb = torch.autograd.grad(out, (a, b), allow_unused=True)
    return (torch.zeros_like(a) if ga is None else ga), (torch.zeros_like(b) if gb is None else gb)


class StokesGrad:
    """Parts C / D: gradient planes (u, v, T, p), their bounds, the pixels a kink leaves out, out8 and its bounds."""

    def __init__(self, d, *, p_pred, loss_type, ls, ld, l2, t_grad, lam=0.0, ra=RA, ih=INV_H, truth=None, thread_adds=8, **mut):
        has_T = t_grad >= 0
        N, H, W = d["u"].shape
        lv = [d[k].clone().requires_grad_(True) for k in ("u", "v", "p", "T")]
        if truth is None:
            ch = [0, 1] + ([2] if p_pred else []) + ([3] if has_T else [])
            truth = d["truth"][:, ch]
        self.truth = truth
        kw = dict(p_pred=p_pred, loss_type=loss_type, ls=ls, ld=ld, l2=l2, has_T=has_T)
        terms, out6 = stokes_terms64(*lv, truth, **kw, **{k: v for k, v in mut.items() if k in ("frame", "swap_norm", "wall0")})

        def grads(t):
            if not t.requires_grad:
                return [torch.zeros_like(x) for x in lv]
            g = torch.autograd.grad(t, lv, retain_graph=True, allow_unused=True)
            return [torch.zeros_like(x) if a is None else a for a, x in zip(g, lv)]
        g_data, g_der, g_mass = (grads(t) for t in terms)
        k = (3.0 if p_pred else 2.0) + (1.0 if has_T else 0.0)
        ut, vt, u, v = truth[:, 0], truth[:, 1], d["u"], d["v"]
        cu, cv = 126.0 / (k * N * (H - 2) * W), 126.0 / (k * N * H * (W - 2))
        wm, wc, wr = 1.0 / (N * (H - 2) * (W - 2)), 1.0 / (N * (H - 2)), 1.0 / (N * (W - 2))

        def mass_form(a, b, wt):                          # sum w (0.5 (a+ + a-) + 0.5 (b+ + b-))
            if loss_type == 0:
                return torch.zeros(())
            m = (0.5 * (a[:, 1:-1, 2:] + a[:, 1:-1, :-2]) + 0.5 * (b[:, 2:, 1:-1] + b[:, :-2, 1:-1])) * wt
            if loss_type == 1:
                return wm * m.sum()
            return wc * (m[:, :, 0].sum() + m[:, :, -1].sum()) + wr * (m[:, 0, :].sum() + m[:, -1, :].sum())

        def der_form(a, b, wu_, wv_):
            if not ld:
                return torch.zeros(())
            return cu * ((a[:, 1:-1, :] + a[:, :-2, :]) * wu_).sum() + cv * ((b[:, :, 1:-1] + b[:, :, :-2]) * wv_).sum()
        one = torch.ones(())
        mag_u, mag_v = _spread(H, W, N, lambda a, b: mass_form(a, b, one) + der_form(a, b, one, one))
        # kinks: a derivative or divergence sign whose argument lies inside its own f32 evaluation error
        ab = torch.abs
        ke_u = ((dy_top(ut) - dy_top(u)).abs() <= K_KINK * U * (ab(ut[:, 1:-1]) + ab(ut[:, :-2]) + ab(u[:, 1:-1]) + ab(u[:, :-2]))).double()
        ke_v = ((dx_left(vt) - dx_left(v)).abs() <= K_KINK * U * (ab(vt[:, :, 1:-1]) + ab(vt[:, :, :-2]) + ab(v[:, :, 1:-1]) + ab(v[:, :, :-2]))).double()
        Dm = 0.5 * (ab(u[:, 1:-1, 2:]) + ab(u[:, 1:-1, :-2])) + 0.5 * (ab(v[:, 2:, 1:-1]) + ab(v[:, :-2, 1:-1]))
        kD = (divergence(u, v).abs() <= K_KINK * U * Dm).double()
        ex_u, ex_v = _spread(H, W, N, lambda a, b: mass_form(a, b, kD) + der_form(a, b, ke_u, ke_v))
        keep_u, keep_v = ex_u == 0, ex_v == 0
        all_ = torch.ones((N, H, W), dtype=torch.bool)
        # planes in the kernels' order: u, v, T, p
        order = (0, 1, 3, 2)
        self.grad = [g_data[i] + g_der[i] + g_mass[i] for i in order]
        mags = [g_data[0].abs() + mag_u, g_data[1].abs() + mag_v, g_data[3].abs(), g_data[2].abs()]
        self.tol = [K_GRAD * U * m for m in mags]
        self.keep = [keep_u, keep_v, all_.clone(), all_.clone()]
        self.out = [float(o.detach()) for o in out6] + [0.0, 0.0]
        self.out_tol = [(K_OUT + thread_adds) * U * abs(o) for o in self.out]
        self.share = max(1.0 - float(keep_u.double().mean()), 1.0 - float(keep_v.double().mean()))
        if lam != 0.0:
            r = Residual(d, lam, ra, ih, p_null=not p_pred)
            e = eta_error(d["T"], d["yc"], d["paras"])[2]
            g = adjoint64(r.sx, r.sy, r.eta, d["scaler"], ra, ih)
            b = adjoint_bound(r.sx, r.sy, r.eta, d["scaler"], ra, ih, e)
            dil = r.dilated()
            for j, i in enumerate(order):
                self.grad[j] = self.grad[j] + g[i]
                self.tol[j] = self.tol[j] + b[i] + U * self.grad[j].abs()
                self.keep[j] = self.keep[j] & ~dil
            cnt = N * (H - 2) * (W - 2)
            mom = (r.sums[0] + r.sums[1]) / cnt
            self.out[6] = mom
            self.out[0] += lam * mom
            self.out_tol[6] = (r.sums_tol[0] + r.sums_tol[1]) / cnt + 2 * U * mom
            self.out_tol[0] += lam * self.out_tol[6] + U * self.out[0]
            self.share = max(self.share, float(dil.double().mean()))
            self.residual = r
        if t_grad <= 0:
            self.grad[2] = torch.zeros_like(self.grad[2])
        if not p_pred:
            self.grad[3] = torch.zeros_like(self.grad[3])


# the covering table of part D2: (route, p_pred, loss_type, ls, ld, l2, t_grad).  Every loss_type, flag, norm and t_grad; l2 with
# the derivative term; l2 with the FluidNet scaled pressure (t_grad -1, ls, p_pred); type 2 through mc_loss_fwd_bwd only
FLAG_CASES = [
    ("fwd_bwd", True, 2, True, True, False, 1),
    ("fwd_bwd", True, 1, True, True, True, 1),          # l2 + derivative
    ("fwd_bwd", True, 2, True, False, True, -1),        # FluidNet: l2 with the scaled pressure, wall weights
    ("fwd_bwd", False, 0, False, True, False, -1),      # FluidNet without pressure: two truth planes, the aliasing quirk
    ("fwd_bwd", False, 1, False, False, False, 0),
    ("fused", True, 1, True, True, False, 1),
    ("fused", True, 0, False, True, True, 0),           # l2 + derivative, T given
    ("fused", False, 1, True, False, False, 1),
    ("fused", True, 1, False, False, False, 1),
]


def finalize64(sums, N, H, W, p_pred, loss_type, ls, ld, t_grad, lam):
    """mc_loss_finalize from the sixteen sums (the slot order of include/mantle_hip.h)."""
    (US, UP, VS, VP, PP, TP, DU, DV, M, MX0, MX1, MY0, MY1, RX, RY) = [float(x) for x in sums[:15]]
    nhw = float(N * H * W)
    lu, lv, tu, tv = (US if ls else UP) / nhw, (VS if ls else VP) / nhw, UP / nhw, VP / nhw
    lp, lT = (PP / nhw if p_pred else 0.0), (TP / nhw if t_grad >= 0 else 0.0)
    if ld:
        lu += DU / (N * (H - 2) * W)
        lv += DV / (N * H * (W - 2))
        if not ls:
            tu, tv = lu, lv
    loss = (lu + lv + lp + lT) / ((3.0 if p_pred else 2.0) + (1.0 if t_grad >= 0 else 0.0))
    mass = M / (N * (H - 2) * (W - 2))
    if loss_type == 1:
        loss += mass
    elif loss_type == 2:
        loss += (MX0 + MX1) / (N * (H - 2)) + (MY0 + MY1) / (N * (W - 2))
    mom = (RX + RY) / (N * (H - 2) * (W - 2))
    if lam != 0.0:
        loss += float(np.float32(lam)) * mom
    return [loss, tu, tv, lp, lT, mass, mom, 0.0]


# ---- curl head ------------------------------------------------------------------------------------------------------------
CURL_SHAPES = [(3, 3), (3, 70), (40, 3), (23, 31), (35, 300)]
A_BOUND, T_LO, T_HI = 4.0, 0.0, 1.5


def curl_head64(a, mag=False):
    """oracle.ref_cpu.curl_head on [N, H, W], restated by index: u = da/dy, v = -da/dx on the interior, replicated outwards,
    antisymmetric across the wall that is normal to the component, zero corners.  mag: all-positive form."""
    sub = (lambda x, y: x + y) if mag else (lambda x, y: x - y)
    neg = 1.0 if mag else -1.0
    u = F.pad((0.5 * sub(a[:, 2:, 1:-1], a[:, :-2, 1:-1])).unsqueeze(1), (1, 1, 1, 1), mode="replicate")[:, 0]
    v = F.pad((neg * 0.5 * sub(a[:, 1:-1, 2:], a[:, 1:-1, :-2])).unsqueeze(1), (1, 1, 1, 1), mode="replicate")[:, 0]
    u = torch.cat((neg * u[:, :, 1:2], u[:, :, 1:-1], neg * u[:, :, -2:-1]), 2)
    v = torch.cat((neg * v[:, 1:2], v[:, 1:-1], neg * v[:, -2:-1]), 1)
    mask = torch.ones_like(a)
    for i in (0, -1):
        for j in (0, -1):
            mask[:, i, j] = 0.0
    return u * mask, v * mask


@functools.lru_cache(maxsize=None)
def curl_case(H, W, N=2, seed=900):
    g = torch.Generator().manual_seed(seed + 7 * H + W)
    a = r32(torch.randn((N, H, W), generator=g, dtype=f64))
    t = r32(torch.rand((N, H, W), generator=g, dtype=f64) * 2.1 - 0.3)             # both clip sides
    t.view(-1)[0::5] = T_LO                                                         # values exactly at the bounds
    t.view(-1)[1::5] = T_HI
    gu, gv, gt = (r32(torch.randn((N, H, W), generator=g, dtype=f64)) for _ in range(3))
    al = (a * A_BOUND).requires_grad_(True)
    tl = t.clone().requires_grad_(True)
    u, v = curl_head64(al)
    tc = torch.clip(tl, T_LO, T_HI)
    ((u * gu).sum() + (v * gv).sum() + (tc * gt).sum()).backward()
    mu, mv = curl_head64((a * A_BOUND).abs(), mag=True)
    am = torch.ones_like(a, requires_grad=True)
    pu, pv = curl_head64(am, mag=True)
    ((pu * gu.abs()).sum() + (pv * gv.abs()).sum()).backward()
    # forward: the difference, x 0.5 (exact), x a_bound: 2 roundings + 1 in hand; backward: the fold adds up to four terms (3),
    # the stencil four more (4), x a_bound (1)
    return dict(a=a, t=t, gu=gu, gv=gv, gt=gt, u=u.detach(), v=v.detach(), tc=tc.detach(), ga=al.grad * A_BOUND, gt_in=tl.grad,
                u_tol=3 * U * mu, v_tol=3 * U * mv, ga_tol=8 * U * A_BOUND * am.grad)


# ---- comparison ---------------------------------------------------------------------------------------------------------
def compare(got, ref, tol):
    """(worst err / tol, mask of failures); a non-finite value fails, tol = 0 asks for equality."""
    got, ref, tol = got.double(), ref.double(), tol.double()
    err = (got - ref).abs()
    bad = ~(err <= tol)
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return (float(r.max()) if r.numel() else 0.0), bad


def check_planes(names, got, ref, tol, keep=None):
    """Failures (strings) and worst err / tol of a list of planes; every pixel of `keep` (all, when None) is compared."""
    out, worst = [], 0.0
    for i, n in enumerate(names):
        t = tol[i] if isinstance(tol[i], torch.Tensor) else torch.full_like(ref[i], float(tol[i]))
        r, bad = compare(got[i], ref[i], t)
        if keep is not None and keep[i] is not None:
            bad = bad & keep[i]
            r = compare(got[i][keep[i]], ref[i][keep[i]], t[keep[i]])[0]
        worst = max(worst, r)
        if bool(bad.any()):
            out.append(f"{n}: {int(bad.sum())} pixels beyond the bound, worst err / tol {r:.3g}")
    return out, worst


def check_residual(r, sx, sy, eta, sums):
    """mc_momentum_residual's outputs against a Residual: eta relative; S exact where |R| exceeds its bound and exactly 0 on the
    outer ring; the two sums."""
    out, worst = [], {}
    f, worst["eta"] = check_planes(["eta_ws"], [eta], [r.eta], [r.eta_rel * r.eta])
    out += f
    f, worst["S"] = check_planes(["sx", "sy"], [sx, sy], [r.sx, r.sy], [0.0, 0.0], [r.keep_x, r.keep_y])
    out += f
    for n, t in (("sx", sx), ("sy", sy)):
        if not bool(((t.abs() == r.c) | (t == 0)).all()):
            out.append(f"{n}: a value that is neither 0 nor +-c")
    w = 0.0
    for n, g, ref, tol in zip(("MC_S_MOMX", "MC_S_MOMY"), sums, r.sums, r.sums_tol):
        e = abs(float(g) - ref)
        w = max(w, e / tol)
        if not e <= tol:
            out.append(f"{n}: {float(g)!r} against {ref!r}, bound {tol:.3e}")
    worst["sums"] = w
    return out, worst


def check_scalars(names, got, ref, tol):
    out, worst = [], 0.0
    for n, g, r, t in zip(names, got, ref, tol):
        e = abs(float(g) - r)
        worst = max(worst, (e / t) if t > 0 else (0.0 if e == 0 else float("inf")))
        if not e <= t:
            out.append(f"{n}: {float(g)!r} against {r!r}, bound {t:.3e}")
    return out, worst


def stored(t):
    """An f64 result as a kernel would leave it in an f32 buffer."""
    return t.to(torch.float32).double()


OUT_NAMES = ("loss", "true_u", "true_v", "loss_p", "loss_T", "mass", "momentum", "zero")
PLANES = ("gu", "gv", "gT", "gp")

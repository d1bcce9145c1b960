"""Case tables, input generators, f64 references and the derived tolerances of tests/test_hip_gn_act.py: the stand-alone
GroupNorm / activation / pooling chain of csrc/groupnorm.hip.  Nothing here touches a device.

References are plain torch in f64 (F.group_norm with eps 1e-5, the exact activations, F.avg_pool2d in floor mode) applied to
the values the kernels read: y after its rounding to the stored type, the gradient tensors in theirs.  Backward references
are autograd of sum_k <g_k, op_k(a)>, op_k = identity (PLAIN), the same on the interior crop of g_k (PADFOLD) or
avg_pool2d(., f) (the _POOL kinds); the per-sample sums (sum dz, sum dz yhat) are the gradients of per-sample copies of beta and
gamma.

The bounds (all first order in 2^-24 = E32, every term written where it is added):
  statistics   a partial is an f32 sum of D values in some order: |error| <= (D + 1) E32 sum |y| (one more rounding for the
               squares); the partials are added in f64.  This gives dmean and dvar and, through rstd = (var + eps)^-1/2, a
               relative bound rel on rstd; both include the rounding of the emitted f32.
  z            z = y sc + sh, sc = rstd gamma, sh = beta - mean rstd gamma: the error of the statistics times |gamma| rstd plus
               six f32 roundings of quantities no larger than Z = |y sc| + |mean sc| + |beta|.  Ez = 0 without GroupNorm.
  a = act(z)   L Ez + E_act.  L: Lipschitz constant of the activation.  E_act, f32: at most LIBM_ULP + 4 roundings (libm
               function, argument scaling, the products and sums around it) of max(|z|, |a|, saturation value); exactly 0
               for identity and relu.  E_act, 16-bit GELU: the MEASURED error of the polynomial (gelu_poly_errors()).
  store        u (|ref| + E) + f on top of the error E before the store; u and f as tests/conv_variants.py defines them
               (UNIT: 2^-8 bf16, 2^-11 f16, 0 f32: half an ulp at the BOTTOM of a binade, the largest relative error of a
               correctly rounded store -- the half-ulp at the top of the binade, 2^-9 / 2^-12, is exceeded by a correct
               kernel on every value just above a power of two; f = 2^-24, the f16 subnormal spacing).
  pooling      mean of the f32 activations: the mean of their bounds + (f^2 + 1) E32 mean(|a| + E), then the store.
  dz = dA g    dA is an f32 sum of the sources (3 E32 sum |source term|), g = act'(z): L' Ez + E_act' (L' bounds |act''|).
  sums         per-pixel bounds added, + (H W + 1) E32 sum |term| for the f32 additions in any order.
  dy           dy = cA dz + cB (y - mean) + cC with cA = rstd gamma, cB = -rstd^2 m2, cC = -rstd m1: the product rule over the
               bounds of every factor + three roundings, then the store.
Kinked activations (relu, selu): elements with |z| < 2^-20 (|y sc| + |sh|) are left out of the dy comparison, and the sums'
bounds grow by |dA| jump for them; SEEDS are chosen so that at most 0.5 % of a case is left out (asserted on the CPU)."""
import functools
import os
import re
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from conv_variants import F16_SPACING, FWD_T, GRAD_T, MC, UNIT, compare       # noqa: F401  (shared with the conv tests)
from pbml_mantle_convection_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = ("f32", "bf16", "mix16")
E32 = 2.0 ** -24
EPS = 1e-5
LIBM_ULP = 4                    # largest error (ulp) the HIP math API documents for erff / expf / tanhf
KINK_REL = 2.0 ** -20
MAX_KINK_SHARE = 0.005
PREFILL = 0.25                  # dgamma / dbeta before mc_gn_act_bwd_finalize / mc_gn_param_grads_batched, which accumulate

SELU_AL, SELU_SC = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
ACTS = ("none", "gelu", "relu", "silu", "tanh", "selu", "elu")
POSTS = {"none": L.POST_NONE, "act": L.POST_ACT, "gn_act": L.POST_GN_ACT}
LIP = {"none": 1.0, "gelu": 1.13, "relu": 1.0, "silu": 1.1, "tanh": 1.0, "selu": SELU_SC * SELU_AL, "elu": 1.0}     # max |act'|
LIP2 = {"none": 0.0, "gelu": 0.8, "relu": 0.0, "silu": 0.5, "tanh": 0.77, "selu": SELU_SC * SELU_AL, "elu": 1.0}    # max |act''|
SAT = {"selu": SELU_SC * SELU_AL, "elu": 1.0}                              # |act(-inf)|
JUMP = {"relu": 1.0, "selu": SELU_SC * (SELU_AL - 1.0)}                    # act'(0+) - act'(0-)


def act64(z, act):
    return {"none": lambda t: t, "gelu": F.gelu, "relu": F.relu, "silu": F.silu, "tanh": torch.tanh, "selu": F.selu,
            "elu": F.elu}[act](z)


def act_grad64(z, act):
    zz = z.detach().clone().requires_grad_()
    return torch.autograd.grad(act64(zz, act).sum(), zz)[0] if act != "none" else torch.ones_like(z)


# ---- the polynomial GELU of the 16-bit modes, measured ------------------------------------------------------------------
def gelu_coefs():
    """(GELU_CDF_COEF, GELU_GRAD_COEF) of csrc/common.h as f32 arrays, lowest order first."""
    src = open(os.path.join(ROOT, "pbml_mantle_convection_amd", "csrc", "common.h")).read()
    out = []
    for name, count in (("GELU_CDF_COEF", 8), ("GELU_GRAD_COEF", 9)):
        m = re.search(r"^#define\s+" + name + r"\s+(.*)$", src, flags=re.M)
        vals = [float(t.strip().rstrip("f")) for t in m.group(1).split(",")]
        assert len(vals) == count, (name, vals)
        out.append(np.array(vals, dtype=np.float32))
    return tuple(out)


def _fma32(a, b, c):
    """f32 fused multiply-add: the product of two f32 is exact in f64 (one rounding of the sum to 53 bits before the one to 24
    differs from a true FMA in the last bit at most, and only on rare ties)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _poly32(z, coef, fused):
    """0.5 + zc P(zc^2) in f32 arithmetic, zc = clamp(z, -4, 4): gelu_cdf_poly2 / gelu_grad_poly2 (fused) or the same Horner
    scheme with separately rounded products and sums."""
    zc = np.clip(z, np.float32(-4.0), np.float32(4.0)).astype(np.float32)
    if fused is None:                        # the polynomial itself: f64 arithmetic on the f32 coefficients
        zd = zc.astype(np.float64)
        return 0.5 + zd * np.polynomial.polynomial.polyval(zd * zd, coef.astype(np.float64))
    w = (zc * zc).astype(np.float32)
    p = np.full_like(zc, coef[-1])
    for k in range(len(coef) - 2, -1, -1):
        p = _fma32(p, w, np.full_like(zc, coef[k])) if fused else ((p * w).astype(np.float32) + coef[k]).astype(np.float32)
    half = np.full_like(zc, 0.5)
    return _fma32(zc, p, half) if fused else ((zc * p).astype(np.float32) + half).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gelu_poly_errors():
    """Largest |error| over 1 600 001 points of [-8, 8] of Phi, GELU = z Phi and GELU' as the 16-bit kernels evaluate them
    (f32, fused and unfused; "exact": the polynomials themselves, in f64), against erf in f64 at the same f32 arguments."""
    cdf, grad = gelu_coefs()
    z = np.linspace(-8.0, 8.0, 1_600_001).astype(np.float32)
    z64 = torch.from_numpy(z.astype(np.float64))
    phi = 0.5 * (1.0 + torch.erf(z64 / 2.0 ** 0.5))
    gelu = z64 * phi
    dgelu = phi + z64 * torch.exp(-0.5 * z64 * z64) / (2.0 * np.pi) ** 0.5
    out = {}
    for fused in (True, False, None):
        tag = "exact" if fused is None else ("fused" if fused else "unfused")
        p = _poly32(z, cdf, fused)
        zp = z.astype(np.float64) * p if fused is None else (z * p).astype(np.float32).astype(np.float64)
        out["cdf_" + tag] = float((torch.from_numpy(p.astype(np.float64)) - phi).abs().max())
        out["fwd_" + tag] = float((torch.from_numpy(zp) - gelu).abs().max())
        out["grad_" + tag] = float((torch.from_numpy(_poly32(z, grad, fused).astype(np.float64)) - dgelu).abs().max())
    out["E_fwd"] = max(out["fwd_fused"], out["fwd_unfused"])
    out["E_grad"] = max(out["grad_fused"], out["grad_unfused"])
    return out


# ---- layout and inputs --------------------------------------------------------------------------------------------------
def to_cb8(x):
    """NCHW -> CB8 [n][ceil(c / 8)][h][w][8], lanes past c zero."""
    n, c, h, w = x.shape
    c8 = (c + 7) // 8
    full = torch.zeros((n, c8 * 8, h, w), dtype=x.dtype)
    full[:, :c] = x
    return full.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def from_cb8(t):
    """CB8 -> [n][c8 * 8][h][w], every lane."""
    n, c8, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)


class Shape(NamedTuple):
    n: int
    c: int
    groups: int
    h: int
    w: int
    seed: int = 0
    sigmas: float = 0.0           # > 0: every (sample, group) is shifted so that its mean is `sigmas` of its standard deviations

    @property
    def cpg(self):
        return self.c // self.groups

    @property
    def c8(self):
        return (self.c + 7) // 8

    @property
    def small(self):
        return self.cpg in (1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def layer_inputs(s):
    """(y, gamma, beta) in f32: channels of different scale and offset, so that the normalisation is not a no-op."""
    g = torch.Generator().manual_seed(9000 + 131 * s.seed + 7 * s.c + 3 * s.h + s.w + 1000 * s.n)
    scale = 0.5 + 1.5 * torch.rand((1, s.c, 1, 1), generator=g)
    offset = 0.7 * torch.randn((1, s.c, 1, 1), generator=g)
    y = torch.randn((s.n, s.c, s.h, s.w), generator=g) * scale + offset
    if s.sigmas:                             # one offset per (sample, group): the spread BETWEEN channels is part of sigma
        yg = y.double().view(s.n, s.groups, -1)
        shift = s.sigmas * yg.std(-1, unbiased=False) - yg.mean(-1)
        y = (y.double() + shift.repeat_interleave(s.cpg, 1).view(s.n, s.c, 1, 1)).float()
    gamma = 1.0 + 0.3 * torch.randn(s.c, generator=g)
    beta = 0.3 * torch.randn(s.c, generator=g)
    return y, gamma, beta


def stored(t, dtype):
    return t.to(dtype).double()


def store_tol(ref, E, dtype):
    return E + UNIT[dtype] * (ref.abs() + E) + (F16_SPACING if dtype == torch.float16 else 0.0)


def per_channel(t, s):
    """[n][groups] -> [n][c][1][1]."""
    return t.repeat_interleave(s.cpg, 1).view(s.n, s.c, 1, 1)


# ---- statistics ---------------------------------------------------------------------------------------------------------
class Stats(NamedTuple):
    mean: torch.Tensor           # [n][groups]
    rstd: torch.Tensor
    dmean: torch.Tensor          # bound on |emitted mean - mean|
    rel: torch.Tensor            # bound on |emitted rstd / rstd - 1|
    sums: torch.Tensor           # [n][c][2]: (sum y, sum y^2) per channel
    dsums: torch.Tensor          # bound on the kernel's f32 partials added in f64


def stats_ref(y64, s, addends, unbiased=False):
    """addends: the largest number of values one f32 partial sums (rows per tile x width)."""
    m = s.cpg * s.h * s.w
    yg = y64.reshape(s.n, s.groups, -1)
    mean, var = yg.mean(-1), yg.var(-1, unbiased=unbiased)
    yc = y64.reshape(s.n, s.c, -1)
    sums = torch.stack([yc.sum(-1), (yc * yc).sum(-1)], -1)
    dsums = torch.stack([(addends + 1) * E32 * yc.abs().sum(-1), (addends + 2) * E32 * (yc * yc).sum(-1)], -1)
    e1 = dsums[..., 0].reshape(s.n, s.groups, -1).sum(-1) / m
    e2 = dsums[..., 1].reshape(s.n, s.groups, -1).sum(-1) / m
    dmean = e1 + E32 * mean.abs()
    dvar = e2 + 2 * mean.abs() * e1 + e1 * e1
    assert bool((dvar < 0.5 * (var + EPS)).all()), "the variance is lost in the f32 partial sums: no bound on rstd"
    rel = dvar / (2 * (var + EPS - dvar)) + E32
    return Stats(mean, (var + EPS).rsqrt(), dmean, rel, sums, dsums)


# ---- forward ------------------------------------------------------------------------------------------------------------
class Fwd(NamedTuple):
    y: torch.Tensor              # the stored y in f64
    z: torch.Tensor
    a: torch.Tensor              # act(z), unrounded
    Ez: torch.Tensor             # bound on the kernel's f32 z
    E: torch.Tensor              # bound on the kernel's f32 a
    tol: torch.Tensor            # ... after the store
    A: torch.Tensor              # |y sc| + |sh|: the scale of the kink rule
    act: str                     # the activation in effect (POST_NONE: none)
    st: object                   # Stats or None
    store: torch.dtype


def act_error(z, a, act, prec):
    if act in ("none", "relu"):
        return torch.zeros_like(z)
    if act == "gelu" and prec != "f32":
        return torch.full_like(z, gelu_poly_errors()["E_fwd"])
    mag = torch.maximum(z.abs(), a.abs())
    if act in SAT:
        mag = torch.maximum(mag, SAT[act] * (z < 0).double())
    return (LIBM_ULP + 4) * E32 * mag


def act_grad_error(z, act, prec):
    if act in ("none", "relu"):
        return torch.zeros_like(z)
    if act == "gelu" and prec != "f32":
        return torch.full_like(z, gelu_poly_errors()["E_grad"])
    return torch.full_like(z, (LIBM_ULP + 4) * E32 * LIP[act])


@functools.lru_cache(maxsize=None)
def forward_ref(s, prec, post, act, addends, mutant=None):
    y, gamma, beta = layer_inputs(s)
    y64, ga, be = stored(y, FWD_T[prec]), gamma.double().view(1, -1, 1, 1), beta.double().view(1, -1, 1, 1)
    st = None
    if post == "gn_act":
        st = stats_ref(y64, s, addends)
        if mutant == "group_shift":          # groups start one channel late (the last group wraps round)
            z = torch.roll(F.group_norm(torch.roll(y64, -1, 1), s.groups, None, None, EPS), 1, 1) * ga + be
        elif mutant == "unbiased":
            mu = stats_ref(y64, s, addends, unbiased=True)
            z = (y64 - per_channel(mu.mean, s)) * per_channel(mu.rstd, s) * ga + be
        else:
            z = F.group_norm(y64, s.groups, gamma.double(), beta.double(), EPS)
        mean, rstd = per_channel(st.mean, s), per_channel(st.rstd, s)
        sc = rstd * ga
        Ez = sc.abs() * (per_channel(st.dmean, s) + (y64 - mean).abs() * per_channel(st.rel, s)) + \
            6 * E32 * ((y64 * sc).abs() + (mean * sc).abs() + be.abs())
        A = (y64 * sc).abs() + (be - mean * sc).abs()
    else:
        z, Ez, A = y64.clone(), torch.zeros_like(y64), y64.abs()
    if post == "none":
        act = "none"
    a = F.gelu(z, approximate="tanh") if mutant == "tanh_gelu" else act64(z, act)
    E = LIP[act] * Ez + act_error(z, a, act, prec)
    return Fwd(y64, z, a, Ez, E, store_tol(a, E, FWD_T[prec]), A, act, st, FWD_T[prec])


def pooled_ref(a, E, f, dtype):
    """AvgPool2d(f) of f32 values within E of a, summed and scaled in f32, stored as dtype."""
    ref = F.avg_pool2d(a, f)
    Ep = F.avg_pool2d(E, f) + (f * f + 1) * E32 * F.avg_pool2d(a.abs() + E, f)
    return ref, store_tol(ref, Ep, dtype)


# ---- gradient sources ---------------------------------------------------------------------------------------------------
class Src(NamedTuple):
    kind: str                    # plain | padfold | padfold_pool | plain_pool
    pad: int = 0
    pool: int = 1
    c8_total: int = 0            # > 0: a slice of a wider tensor of c8_total channel blocks, starting at block cb_off
    cb_off: int = 0

    @property
    def mc_kind(self):
        return {"plain": L.GSRC_PLAIN, "padfold": L.GSRC_PADFOLD, "padfold_pool": L.GSRC_PADFOLD_POOL,
                "plain_pool": L.GSRC_PLAIN_POOL}[self.kind]

    @property
    def halo(self):
        return self.pad if self.kind.startswith("padfold") else 0

    @property
    def f(self):
        return self.pool if self.kind.endswith("pool") else 1


GARBAGE = 3.0e4                  # around a padfold interior: any read of the halo is far outside every bound


@functools.lru_cache(maxsize=None)
def source_tensor(s, src, k, prec):
    """Source k of a case as it lies in memory, in the gradient type: [n][channels][hs + 2 pad][ws + 2 pad] with a garbage halo;
    a slice's tensor has c8_total * 8 channels, all of them data (the neighbours belong to other layers)."""
    if src.c8_total:                         # every slice of a case reads the SAME wider tensor, whichever source it is
        return wide_tensor(s, src._replace(cb_off=0), prec)
    return _source_tensor(s, src, k, prec)


@functools.lru_cache(maxsize=None)
def wide_tensor(s, src, prec):
    return _source_tensor(s, src, 99, prec)


def _source_tensor(s, src, k, prec):
    g = torch.Generator().manual_seed(77000 + 977 * s.seed + 31 * k + 7 * s.h + s.w + 13 * src.pool + src.pad)
    hs, ws, p = s.h // src.f, s.w // src.f, src.halo
    ch = src.c8_total * 8 if src.c8_total else s.c
    t = GARBAGE * (1.0 + torch.rand((s.n, ch, hs + 2 * p, ws + 2 * p), generator=g))
    t[:, :, p:p + hs, p:p + ws] = torch.randn((s.n, ch, hs, ws), generator=g)
    return t.to(GRAD_T[prec])


def source_values(s, src, k, prec, shift=0):
    """The values the layer's backward reads from source k: [n][c][hs][ws] in f64.  shift: the padfold-offset mutant."""
    t = source_tensor(s, src, k, prec).double()
    p, c0 = src.halo - shift, src.cb_off * 8
    hs, ws = s.h // src.f, s.w // src.f
    return t[:, c0:c0 + s.c, p:p + hs, p:p + ws]


def adjoint(s, srcs, vals, mutant=None):
    """dA = d/da sum_k <g_k, op_k(a)> by autograd (linear in a: evaluated at a = 0)."""
    a = torch.zeros((s.n, s.c, s.h, s.w), dtype=torch.float64, requires_grad=True)
    loss = 0.0
    for src, g in zip(srcs, vals):
        if src.f == 1:
            loss = loss + (g * a).sum()
        elif mutant == "pool_unscaled":
            loss = loss + (g * F.avg_pool2d(a, src.f)).sum() * src.f * src.f
        elif mutant == "pool_trailing":      # ceil mode: the trailing rows and columns are pooled (and fed) too
            op = F.avg_pool2d(a, src.f, ceil_mode=True, count_include_pad=False)
            gg = F.pad(g, (0, op.shape[3] - g.shape[3], 0, op.shape[2] - g.shape[2]), mode="replicate")
            loss = loss + (gg * op).sum()
        else:
            loss = loss + (g * F.avg_pool2d(a, src.f)).sum()
    return torch.autograd.grad(loss, a)[0]


# ---- backward -----------------------------------------------------------------------------------------------------------
class Bwd(NamedTuple):
    dy: torch.Tensor
    dy_tol: torch.Tensor
    keep: torch.Tensor           # elements compared (the kink rule leaves the others out)
    sums: torch.Tensor           # [n][c][2] = (sum dz, sum dz yhat)                     (GroupNorm only, like the rest)
    sums_tol: torch.Tensor
    m12: torch.Tensor            # [n][groups][2]
    m12_tol: torch.Tensor
    dparam: torch.Tensor         # [2][c] = (dbeta, dgamma) INCLUDING the prefill
    dparam_tol: torch.Tensor
    parts: dict                  # intermediate f64 tensors for the mutants of the CPU tests


@functools.lru_cache(maxsize=None)
def backward_ref(s, prec, post, act, srcs, addends):
    fw = forward_ref(s, prec, post, act, addends)
    act = fw.act
    gt = GRAD_T[prec]
    _, gamma, beta = layer_inputs(s)
    vals = [source_values(s, src, k, prec) for k, src in enumerate(srcs)]
    # autograd: per-sample copies of gamma and beta give the per-sample sums
    y = fw.y.clone().requires_grad_()
    gam = gamma.double().expand(s.n, s.c).clone().requires_grad_()
    bet = beta.double().expand(s.n, s.c).clone().requires_grad_()
    if post == "gn_act":
        z = F.group_norm(y, s.groups, None, None, EPS) * gam[:, :, None, None] + bet[:, :, None, None]
    else:
        z = y * 1.0
    z.retain_grad()
    a = act64(z, act)
    a.retain_grad()
    loss = 0.0
    for src, g in zip(srcs, vals):
        loss = loss + (g * (F.avg_pool2d(a, src.f) if src.f > 1 else a)).sum()
    loss.backward()
    dy, dA, dz = y.grad, a.grad, z.grad
    assert torch.allclose(dA, adjoint(s, srcs, vals), rtol=1e-12, atol=0.0)
    dAabs = adjoint(s, srcs, [v.abs() for v in vals])
    gp = act_grad64(fw.z, act)
    # dz = dA act'(z)
    E_dA = 3 * E32 * dAabs
    E_g = LIP2[act] * fw.Ez + act_grad_error(fw.z, act, prec)
    E_dz = dA.abs() * E_g + gp.abs() * E_dA + E_dA * E_g + E32 * dz.abs()
    kink = (fw.z.abs() < KINK_REL * fw.A) if act in JUMP else torch.zeros_like(fw.z, dtype=torch.bool)
    flip = kink.double() * dA.abs() * JUMP.get(act, 0.0)
    parts = dict(dA=dA, gp=gp, z=fw.z, y=fw.y, vals=vals, kink=kink)
    if post != "gn_act":                     # dy = 1 dz + (0 (y - 0) + 0): exact
        return Bwd(dy, store_tol(dy, E_dz, gt), ~kink, None, None, None, None, None, None, parts)
    st = fw.st
    mean, rstd, dmean, rel = (per_channel(t, s) for t in (st.mean, st.rstd, st.dmean, st.rel))
    ga = gamma.double().view(1, -1, 1, 1)
    t = fw.y - mean
    yh = t * rstd
    E_yh = rstd * (dmean + t.abs() * rel) + 2 * E32 * yh.abs()
    P = s.h * s.w
    t2 = dz * yh
    E_t2 = E_dz * (yh.abs() + E_yh) + dz.abs() * E_yh + 2 * E32 * t2.abs()
    hw = (2, 3)
    sums = torch.stack([bet.grad, gam.grad], -1)
    assert torch.allclose(sums[..., 0], dz.sum(hw)) and torch.allclose(sums[..., 1], t2.sum(hw))
    B1 = (E_dz + flip).sum(hw) + (P + 1) * E32 * (dz.abs() + E_dz).sum(hw)
    B2 = (E_t2 + flip * (yh.abs() + E_yh)).sum(hw) + (P + 1) * E32 * (t2.abs() + E_t2).sum(hw)
    sums_tol = torch.stack([B1, B2], -1)
    mag = torch.stack([dz.abs().sum(hw), t2.abs().sum(hw)], -1) + sums_tol          # [n][c][2]: bound on |the f32 sums|
    # dbeta / dgamma: the prefill plus the samples in order, in f32
    dparam = PREFILL + sums.sum(0).t()
    dparam_tol = sums_tol.sum(0).t() + (s.n + 2) * E32 * (PREFILL + mag.sum(0).t())
    # m12 = sum_c gamma_c sums_c / M over the channels of a group
    M = s.cpg * P
    gw = gamma.double().view(1, -1, 1)
    m12 = (gw * sums).view(s.n, s.groups, s.cpg, 2).sum(2) / M
    m12_tol = ((gw.abs() * sums_tol).view(s.n, s.groups, s.cpg, 2).sum(2) +
               (s.cpg + 3) * E32 * (gw.abs() * mag).view(s.n, s.groups, s.cpg, 2).sum(2)) / M
    m1, m2 = per_channel(m12[..., 0], s), per_channel(m12[..., 1], s)
    t_m1, t_m2 = per_channel(m12_tol[..., 0], s), per_channel(m12_tol[..., 1], s)
    cA, cB, cC = rstd * ga, -rstd * rstd * m2, -rstd * m1
    E_cA = cA.abs() * (rel + E32)
    E_cB = rstd * rstd * t_m2 * (1 + rel) ** 2 + cB.abs() * (2 * rel + rel * rel + 2 * E32)
    E_cC = rstd * t_m1 * (1 + rel) + cC.abs() * (rel + E32)
    E_t = dmean + E32 * t.abs()
    E_dy = cA.abs() * E_dz + dz.abs() * E_cA + E_cA * E_dz + cB.abs() * E_t + t.abs() * E_cB + E_cB * E_t + E_cC + \
        3 * E32 * ((cA * dz).abs() + (cB * t).abs() + cC.abs())
    parts.update(rstd=rstd, ga=ga, yh=yh, m1=m1, m2=m2, mean=mean)
    return Bwd(dy, store_tol(dy, E_dy, gt), ~kink, sums, sums_tol, m12, m12_tol, dparam, dparam_tol, parts)


def manual_dy(s, parts, dA=None, gp=None, drop_m2=False):
    """dy = rstd (gamma dz - m1 - yhat m2) from the parts of a GroupNorm Bwd, with some of them replaced: the CPU tests'
    mutants (with nothing replaced it must reproduce autograd)."""
    dA = parts["dA"] if dA is None else dA
    gp = parts["gp"] if gp is None else gp
    dz = dA * gp
    M = s.cpg * s.h * s.w
    g = parts["ga"]

    def group_mean(v):
        return per_channel((g * v).sum((2, 3)).view(s.n, s.groups, s.cpg).sum(2) / M, s)
    m1, m2 = group_mean(dz), group_mean(dz * parts["yh"])
    return parts["rstd"] * (g * dz - m1 - (0.0 if drop_m2 else parts["yh"] * m2))


# ---- the case tables ----------------------------------------------------------------------------------------------------
SWEEP = Shape(2, 12, 3, 9, 11)               # 4 channels per group, ragged second channel block, odd H and W
TILES = 4                                    # mc_gn_partials tiles of every case below but the statistics cases


def addends_of(s, tiles=TILES):
    t = min(tiles, s.h)
    return -(-s.h // t) * s.w


def tiles_of(s, tiles=TILES):
    return min(tiles, s.h)


SIGMA_SHAPE = Shape(2, 8, 2, 9, 11, sigmas=8.0)
#             shape                          tiles
STAT_CASES = [
    (Shape(2, 8, 8, 9, 11), 4),              # 1 channel per group
    (Shape(2, 8, 4, 9, 11), 4),              # 2
    (Shape(2, 8, 2, 9, 11), 9),              # 4, one row per tile
    (Shape(2, 16, 2, 9, 11), 4),             # 8
    (Shape(2, 16, 1, 9, 11), 4),             # 16
    (Shape(2, 12, 4, 9, 11), 4),             # 3: general path, ragged channel block
    (Shape(2, 12, 2, 9, 11), 4),             # 6: general path
    (Shape(2, 12, 3, 3, 11), 8),             # tiles > H: mc_gn_partials refuses; mc_gn_finalize over 3 filled + 5 zero slots
    (Shape(2, 12, 3, 9, 11), 1),             # one tile
    (Shape(2, 16, 2, 70, 13), 65),           # 8 lanes per channel: one 8-in-flight round (t < 64) + the tail slot 64
    (Shape(2, 16, 1, 70, 13), 65),           # 4 lanes per channel: two rounds + the tail
    (SIGMA_SHAPE, 4),                        # group mean = 8 sigma: ss / m = 65 var, the difference cancels 6 bits of the f32 partials
]

# forward shapes: (shape, pool, a present)
FWD_SHAPES = [
    (Shape(2, 8, 2, 40, 54), 1, True),       # 2160 vectors: two blocks of 2048, grid-stride loop
    (Shape(2, 8, 2, 9, 12), 2, True),        # even W, odd H: row pairs in the 16-bit types, last row unpaired
    (Shape(2, 8, 2, 9, 11), 2, True),        # odd W: block form
    (Shape(2, 8, 2, 1, 12), 2, True),        # H = 1: no row pair, block form, empty pooled tensor
    (Shape(2, 12, 3, 9, 11), 4, True),       # trailing row and columns: activated, not pooled
    (Shape(2, 8, 2, 9, 12), 2, False),       # a == NULL
    (Shape(2, 8, 2, 9, 12), 4, False),
]
SMALL_SHAPES = [Shape(2, 8, 8, 9, 12), Shape(2, 8, 4, 9, 12), Shape(2, 12, 3, 9, 12), Shape(2, 8, 1, 9, 11),
                Shape(2, 12, 3, 9, 11)]
POOL_SHAPE = Shape(2, 12, 3, 9, 11)          # mc_avgpool_fwd, f in 2, 3, 4: H and W multiples of none of them
POOL_FACTORS = (2, 3, 4)

SRC_SWEEP = (Src("padfold", 2), Src("plain"))
SLICE_SHAPE = Shape(2, 8, 2, 9, 11, seed=1)  # one channel block: blocks 1 and 2 of a three-block tensor
RAGGED_SLICE = Shape(2, 12, 3, 9, 11, seed=1)  # blocks 1 and 2 of the three: lanes 4-7 of the last hold another layer's data
# (shape, sources); the 16-bit types take the compile-time kinds GK = 2, 1, 3 for the first three, the run-time path after
SOURCE_CASES = [
    (SWEEP, (Src("plain"),)),
    (SWEEP, (Src("padfold", 1),)),
    (SWEEP, (Src("padfold", 2), Src("padfold_pool", 2, 2))),       # 9 x 11 -> 4 x 5: last row and column get no pool gradient
    (SWEEP, (Src("plain_pool", 0, 4),)),
    (SWEEP, (Src("plain"), Src("plain_pool", 0, 2))),
    (SLICE_SHAPE, (Src("plain", 0, 1, 3, 1), Src("plain", 0, 1, 3, 2))),      # two slices of one wider tensor
    (SLICE_SHAPE, (Src("plain", 0, 1, 3, 2), Src("padfold", 2))),            # a slice and a whole tensor
    (RAGGED_SLICE, (Src("padfold", 1), Src("plain", 0, 1, 3, 1))),           # a whole tensor and a ragged slice
]
# apply rows per block 32 / 16 / 8 (W <= 32, <= 256, > 256) with a ragged last block; reduce with H no multiple of the block
# count, and with fewer rows than blocks (mc_gn_bwd_blocks = ceil(H W / 2048))
LAUNCH_SHAPES = [Shape(2, 8, 2, 33, 31), Shape(2, 8, 2, 17, 33), Shape(2, 8, 2, 9, 257), Shape(2, 8, 2, 45, 70),
                 Shape(2, 8, 2, 2, 2100)]
GENERAL_SHAPES = [Shape(2, 12, 4, 9, 11, seed=2), Shape(2, 16, 1, 9, 11, seed=2)]        # 3 and 16 channels per group
CHUNK_SHAPE = Shape(257, 8, 2, 4, 4)         # N crosses the 256-sample LDS chunk of k_gn_bwd_finalize
CHUNK_BLOCKS = (1, 3, 5)                     # slots per sample: the four-wave split of k_gn_bwd_finalize_n with empty waves


def backward_cases():
    """Every (shape, post, act, sources) the GPU tests run a backward for: the kink share is asserted over these."""
    out = [(SWEEP, post, act, SRC_SWEEP) for post in POSTS for act in ACTS]
    out += [(s, "gn_act", act, srcs) for s, srcs in SOURCE_CASES for act in ("gelu", "selu")]
    out += [(s, "gn_act", "gelu", (Src("plain"),)) for s in LAUNCH_SHAPES]
    out += [(s, "gn_act", "selu", SRC_SWEEP) for s in GENERAL_SHAPES]
    return out


@functools.lru_cache(maxsize=None)
def chunk_partials(blocks):
    """Host-made reduce partials [257][blocks][8][2] and gamma for the finalize kernels alone."""
    g = torch.Generator().manual_seed(5100 + blocks)
    s = CHUNK_SHAPE
    return torch.randn((s.n, blocks, s.c, 2), generator=g), 1.0 + 0.3 * torch.randn(s.c, generator=g)


def finalize_ref(part, gamma, s):
    """(m12, tol, dparam [2][c] incl. prefill, tol, chan_sums, tol: the rounding to f32 and one more E32 for the f64 additions
    of the per-wave subtotals, the (D + 1) rule of the other sums) of partials summed in f64 and rounded to f32 (m12 again after the division;
    the one-launch route weighs in f32: cpg + 3 roundings), then added sample by sample in f32."""
    p = part.double()
    sums, mag = p.sum(1), p.abs().sum(1)                       # [n][c][2]
    M = s.cpg * s.h * s.w
    gw = gamma.double().view(1, -1, 1)
    m12 = (gw * sums).view(s.n, s.groups, s.cpg, 2).sum(2) / M
    m12_tol = (s.cpg + 3) * E32 * (gw.abs() * mag).view(s.n, s.groups, s.cpg, 2).sum(2) / M
    dparam = PREFILL + sums.sum(0).t()
    dparam_tol = (s.n + 2) * E32 * (PREFILL + mag.sum(0).t())
    return m12, m12_tol, dparam, dparam_tol, sums, 2 * E32 * mag

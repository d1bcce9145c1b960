"""The stand-alone GroupNorm / activation / pooling kernels of csrc/groupnorm.hip against f64, straight through the C ABI, at
the shapes where their index arithmetic, launch shapes and dispatch can go wrong (tests/gn_cases.py: the case tables, the f64
references and the derived bounds).

  CPU only   the polynomial GELU of the 16-bit modes has the error csrc/common.h states; the kink rule leaves out at most
             0.5 % of any case; the host-side refusals return the documented codes; the comparison rejects nine mutants; the 8 sigma case has |mean| >= 7.5 sigma
  GPU        statistics (mc_gn_partials, mc_gn_finalize[_coef]); forward (mc_gn_act_fwd in its block and row-pair forms,
             mc_gn_act_fwd_small, mc_avgpool_fwd); backward (reduce -> finalize -> apply, mc_gn_act_bwd_small, the _n and _dz
             finalize forms, mc_gn_param_grads_batched)

Every buffer a launch writes is prefilled with NaN and lies between sentinel bands, padfold interiors lie in garbage, lanes past
c of every CB8 output must be exactly zero, and no MC_GN_* / MANTLE_* variable is set: the default launch shapes are tested.

Measured polynomial errors (1 600 001 points of [-8, 8]; f32 with FMAs as the kernels evaluate / f32 with separate roundings /
the polynomials themselves in f64): Phi 4.59e-5 / 4.64e-5 / 4.48e-5, GELU 1.82e-4 / 1.84e-4 / 1.78e-4, GELU' 5.02e-4 /
5.09e-4 / 4.91e-4.  The bounds use the larger f32 figure: E_fwd = 1.84e-4, E_grad = 5.09e-4.

Every GPU test prints its worst err / tol per kernel family (`pytest -s`).  On MI355X, worst over all cases (f32 / bf16 / mix16):
  mc_gn_partials              sums 0.083 / 0.044 / 0.079
  mc_gn_finalize[_coef]       mean, rstd, chan_mean 0.093 / 0.075 / 0.089; coef4 rows equal bit for bit
  mc_gn_act_fwd               a 0.234 / 0.987 / 0.984, pooled 0.037 / 0.955 / 0.936
  mc_gn_act_fwd_small         a 0.063 / 0.990 / 0.969, pooled 0.044 / 0.967 / 0.970; statistics, a and pooled equal the other forms'
  mc_avgpool_fwd              0.421 / 0.988 / 0.985
  mc_gn_act_bwd_reduce        sums 0.007 / 0.095 / 0.096
  mc_gn_act_bwd_finalize      m12, dgamma, dbeta 0.006 / 0.053 / 0.053; host-made partials, N = 257: 0.128
  mc_gn_act_bwd_finalize_n    m12, chan_sums 0.007 / 0.095 / 0.096; N = 257: chan_sums 0.50, m12 0.128
  mc_gn_param_grads_batched   0.006 / 0.053 / 0.053
  mc_gn_act_bwd_apply         dy 0.634 / 0.996 / 0.996
  mc_gn_act_bwd_small         dy 0.036 / 0.976 / 0.986
  the _dz finalize forms      m12 0.002; dz_coef rows equal bit for bit
A 16-bit output sits just under 1 by construction: its error is the final rounding, at worst u |ref| of the u (|ref| + E) + E
allowed (the sums of the 16-bit GELU cases reach 0.10: the polynomial's error is a smooth function of z, not a random
rounding, so it cancels less in a sum).  The 8 sigma statistics case stays at 0.03 (rstd) in every type.  The f32 figures above 0.1:
  a 0.234 and dy 0.248 / 0.634 come from the post = ACT cases, where Ez = 0 and the bound is nothing but the activation's own
  LIBM_ULP + 4 roundings (dy with identity / relu: the four roundings of the two-source sum and the product, of which the
  kernel makes one: 0.25).  a stays at a quarter of the eight; silu' = s (1 + z (1 - s)) comes closest, because the
  rounding of 1 - s is multiplied by z (|z| up to 4 here): 0.634.
  mc_avgpool_fwd 0.421: the bound is f^2 + 1 roundings of mean |a|, and the kernel makes f^2 additions and one product.
  N = 257, host-made partials: chan_sums is one rounding of an f64 sum to f32 against a bound of 2 x 2^-24 sum |partial| (the
  rounding, and one more for the f64 additions of the subtotals): an element whose partials have one sign and whose sum
  rounds by half an ulp reaches 0.50 by construction; m12 0.128 is one rounding of the cpg + 3 allowed.
mc_gn_partials refuses tiles > H (MC_EINVAL, asserted on the host); the `tiles > H` case therefore runs mc_gn_finalize with
eight slots over the three filled by mc_gn_partials and five of zeros, as a conv epilogue with rowless tiles leaves them."""
import ctypes as C
import functools
import os

import pytest
import torch

import gn_cases as G
from pbml_mantle_convection_amd import _lib as L

DEV = "cuda:0"
SENTINEL = 0x7B
gpu = pytest.mark.gpu
ACT_ID = {a: L.ACTS[a] for a in G.ACTS}


def stored_as(t, dtype):
    """An f64 result as a kernel would leave it: through f32 into the stored type."""
    return t.to(torch.float32).to(dtype).double()


def fails(got, ref, tol, keep=None):
    bad = G.compare(got, ref, tol)[1]
    return bool((bad if keep is None else bad & keep).any())


# ---- CPU only -----------------------------------------------------------------------------------------------------------
def test_polynomial_gelu_error_is_as_stated():
    """The measured maxima (they are the E_act of every 16-bit GELU bound) stay below the issue's 2e-4 / 5.5e-4, and the
    comment in csrc/common.h states them."""
    e = G.gelu_poly_errors()
    print("\npolynomial GELU, |error| on [-8, 8]: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["E_fwd"] < 2e-4 and e["E_grad"] < 5.5e-4
    assert e["fwd_exact"] > 1.7e-4 and e["grad_fused"] > 5.0e-4 and e["cdf_exact"] > 4.3e-5        # (the earlier statement was low)
    src = open(os.path.join(G.ROOT, "pbml_mantle_convection_amd", "csrc", "common.h")).read()
    for k, (v, text) in {"cdf": (4.7e-5, "4.7e-5"), "fwd": (1.85e-4, "1.85e-4"), "grad": (5.1e-4, "5.1e-4")}.items():
        assert text in src, f"csrc/common.h does not state {text}"
        assert max(e[k + "_fused"], e[k + "_unfused"], e[k + "_exact"]) <= v


@pytest.mark.parametrize("prec", G.PRECS)
def test_kink_rule_leaves_out_at_most_half_a_percent(prec):
    worst = 0.0
    for s, post, act, srcs in G.backward_cases():
        b = G.backward_ref(s, prec, post, act, srcs, G.addends_of(s))
        share = 1.0 - float(b.keep.double().mean())
        worst = max(worst, share)
        assert share <= G.MAX_KINK_SHARE, (s, post, act, share)
        if act not in G.JUMP or post == "none":
            assert share == 0.0
    print(f"\n[{prec}] largest share left out of a dy comparison: {worst:.5f}")


def test_host_side_refusals():
    """These checks return before any launch (no device needed): the code the source returns for each."""
    lib = L.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    GN, gelu, f32 = L.POST_GN_ACT, L.ACTS["gelu"], L.MC_F32
    EINVAL, EUNSUP = -1, -2

    def src(kind=L.GSRC_PLAIN, pad=0, pool=1, c8_total=0, cb_off=0):
        return C.byref(L.GradSrc(p, kind, pad, 0, pool, 9, 11, c8_total, cb_off))

    def fwd(c=12, groups=3, post=GN, act=gelu, pool=1):
        return lib.mc_gn_act_fwd(p, 2, c, 9, 11, groups, p, p, p, post, act, pool, f32, p, p, None)

    def small(groups=3, pool=1):
        return lib.mc_gn_act_fwd_small(p, p, 4, 2, 12, 9, 11, groups, G.EPS, p, p, gelu, pool, f32, p, p, p, None)

    def reduce(groups=3, post=GN, act=gelu, g0=None):
        return lib.mc_gn_act_bwd_reduce(p, 2, 12, 9, 11, groups, p, p, p, post, act, f32, g0 or src(), None, p, None)

    def apply(groups=3, post=GN, act=gelu, g0=None):
        return lib.mc_gn_act_bwd_apply(p, 2, 12, 9, 11, groups, p, p, p, p, post, act, f32, g0 or src(), None, p, None)

    def bsmall(groups=3, g0=None):
        return lib.mc_gn_act_bwd_small(p, 2, 12, 9, 11, groups, p, p, p, gelu, f32, g0 or src(), None, p, p, None)

    # c % groups != 0
    assert lib.mc_gn_finalize(p, 2, 4, 12, 5, 99, G.EPS, p, None, None) == EINVAL
    assert lib.mc_gn_finalize_coef(p, 2, 4, 12, 5, 99, G.EPS, p, p, p, p, None) == EINVAL
    assert fwd(groups=5) == EINVAL and small(groups=5) == EINVAL and reduce(groups=5) == EINVAL
    assert apply(groups=5) == EINVAL and bsmall(groups=5) == EINVAL
    assert lib.mc_gn_act_bwd_finalize(p, 2, 1, 12, 5, 99, p, p, p, p, None) == EINVAL
    assert lib.mc_gn_act_bwd_finalize_n(p, 2, 1, 12, 5, 99, p, p, p, None) == EINVAL
    # pool 3 (and pool 4 in the one-launch form)
    assert fwd(pool=3) == EUNSUP and small(pool=3) == EUNSUP and small(pool=4) == EUNSUP
    # the one-launch forms and finalize_n with 3 channels per group
    assert small(groups=4) == EUNSUP and bsmall(groups=4) == EUNSUP
    assert lib.mc_gn_act_bwd_finalize_n(p, 2, 1, 12, 4, 99, p, p, p, None) == EUNSUP
    assert lib.mc_gn_act_bwd_finalize_n_dz(p, 2, 1, 12, 4, 99, p, p, p, p, p, None) == EUNSUP
    # a padfold source with pad 3
    for kind in (L.GSRC_PADFOLD, L.GSRC_PADFOLD_POOL):
        assert reduce(g0=src(kind, 3, 2)) == EUNSUP and apply(g0=src(kind, 3, 2)) == EUNSUP and bsmall(g0=src(kind, 3, 2)) == EUNSUP
    # a slice that starts behind its tensor
    for off in (3, 4):
        assert reduce(g0=src(c8_total=3, cb_off=off)) == EINVAL and apply(g0=src(c8_total=3, cb_off=off)) == EINVAL
        assert bsmall(g0=src(c8_total=3, cb_off=off)) == EINVAL
    # post or act out of range
    for post, act in ((3, gelu), (-1, gelu), (GN, 7), (GN, -1), (L.POST_ACT, 7)):
        assert fwd(post=post, act=act) == EINVAL and apply(post=post, act=act) == EINVAL and reduce(post=post, act=act) == EINVAL
    # the reduction exists for GroupNorm layers only
    assert reduce(post=L.POST_ACT) == EINVAL and reduce(post=L.POST_NONE) == EINVAL
    # more tiles than rows
    assert lib.mc_gn_partials(p, 2, 12, 3, 11, f32, 8, p, None) == EINVAL


@pytest.mark.parametrize("prec", G.PRECS)
def test_eight_sigma_case_is_eight_sigma(prec):
    """The stored values of the cancellation case: every (sample, group) has |mean| >= 7.5 sigma, so ss / m >= 57 var."""
    s = G.SIGMA_SHAPE
    assert any(c is s for c, _ in G.STAT_CASES)
    yg = G.stored(G.layer_inputs(s)[0], G.FWD_T[prec]).view(s.n, s.groups, -1)
    ratio = yg.mean(-1).abs() / yg.std(-1, unbiased=False)
    print(f"\n[{prec}] |group mean| / sigma: {[round(float(v), 2) for v in ratio.flatten()]}")
    assert bool((ratio >= 7.5).all())


BWD_TEETH = (G.SWEEP, "gn_act", "selu", (G.Src("padfold", 2), G.Src("padfold_pool", 2, 2)))


@pytest.mark.parametrize("prec", G.PRECS)
def test_comparison_has_teeth(prec):
    """Each mutant of the reference, rounded to the stored type like a kernel's output, fails the comparison the GPU tests use;
    the reference itself passes."""
    s, add = G.SWEEP, G.addends_of(G.SWEEP)
    ft, gt = G.FWD_T[prec], G.GRAD_T[prec]
    ref = G.forward_ref(s, prec, "gn_act", "selu", add)
    assert not fails(stored_as(ref.a, ft), ref.a, ref.tol)
    hole = stored_as(ref.a, ft)
    hole[-1, -1, -1, -1] = float("nan")                       # an element the kernel never wrote
    assert int(G.compare(hole, ref.a, ref.tol)[1].sum()) == 1
    for mutant in ("group_shift", "unbiased"):
        mut = G.forward_ref(s, prec, "gn_act", "selu", add, mutant)
        assert fails(stored_as(mut.a, ft), ref.a, ref.tol), mutant
    unb = G.stats_ref(ref.y, s, add, unbiased=True)
    assert bool(((unb.rstd - ref.st.rstd).abs() > ref.st.rel * ref.st.rstd).all())
    if prec == "f32":
        gref = G.forward_ref(s, prec, "gn_act", "gelu", add)
        assert not fails(stored_as(gref.a, ft), gref.a, gref.tol)
        assert fails(stored_as(G.forward_ref(s, prec, "gn_act", "gelu", add, "tanh_gelu").a, ft), gref.a, gref.tol)
    # pooled tensor: a scale of 1 / f instead of 1 / f^2
    pr, pt = G.pooled_ref(ref.a, ref.E, 2, ft)
    assert not fails(stored_as(pr, ft), pr, pt) and fails(stored_as(2 * pr, ft), pr, pt)

    _, post, act, srcs = BWD_TEETH
    b = G.backward_ref(s, prec, post, act, srcs, add)
    P = b.parts
    assert torch.allclose(G.manual_dy(s, P), b.dy, rtol=1e-9, atol=1e-12)
    assert not fails(stored_as(b.dy, gt), b.dy, b.dy_tol, b.keep)
    shifted = [G.source_values(s, src, k, prec, shift=1 if src.halo else 0) for k, src in enumerate(srcs)]
    mutants = {
        "elu' for selu'": G.manual_dy(s, P, gp=G.act_grad64(P["z"], "elu")),
        "pool adjoint without 1 / f^2": G.manual_dy(s, P, dA=G.adjoint(s, srcs, P["vals"], "pool_unscaled")),
        "pool adjoint feeds the trailing row": G.manual_dy(s, P, dA=G.adjoint(s, srcs, P["vals"], "pool_trailing")),
        "padfold read at (p - 1, p - 1)": G.manual_dy(s, P, dA=G.adjoint(s, srcs, shifted)),
        "dy without m2 yhat": G.manual_dy(s, P, drop_m2=True),
    }
    for name, mut in mutants.items():
        assert fails(stored_as(mut, gt), b.dy, b.dy_tol, b.keep), f"{name} passes: the inputs are too tame"
    # the trailing-row mutant differs from the reference in the last row / column only where the other terms do not carry it
    # over through m1, m2: it must fail there
    bad = G.compare(stored_as(mutants["pool adjoint feeds the trailing row"], gt), b.dy, b.dy_tol)[1]
    assert bool(bad[:, :, -1, :].any()) and bool(bad[:, :, :, -1].any())


# ---- GPU ----------------------------------------------------------------------------------------------------------------
class Guarded:
    """A tensor between two sentinel bands inside one larger allocation (restated from tests/test_hip_dropout.py; the pointer
    is taken from the allocation, so that an empty tensor still has one)."""

    def __init__(self, shape, dtype, fill=float("nan"), guard_bytes=65536):
        n = 1
        for v in shape:
            n *= int(v)
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        if fill is not None and n:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.g

    def cpu(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[:self.g] == SENTINEL).all()), f"{what}: bytes BEFORE the buffer were overwritten"
        assert bool((self.raw[self.g + self.nbytes:] == SENTINEL).all()), f"{what}: bytes BEHIND the buffer were overwritten"
        return self.t.cpu()


class Report:
    """Worst err / tol per kernel family of one test."""

    def __init__(self, tag):
        self.tag, self.worst = tag, {}

    def within(self, family, what, got, ref, tol, keep=None):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        tol = tol.expand_as(ref)
        r, bad = G.compare(got, ref, tol)                       # (the comparison the CPU tests put the mutants through)
        if keep is not None:
            r, bad = G.compare(got[keep], ref[keep], tol[keep])[0], bad & keep
        self.worst[family] = max(self.worst.get(family, 0.0), r)
        if bad.any():
            idx = [tuple(int(v) for v in i) for i in bad.nonzero()[:6]]
            raise AssertionError(f"[{self.tag}] {what}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/tol {r:.3f}, "
                                 f"first at {idx}: got {[float(got[i]) for i in idx]}, ref {[float(ref[i]) for i in idx]}")

    def show(self):
        print(f"\n[{self.tag}] worst err/tol: " + ", ".join(f"{k} {v:.3g}" for k, v in self.worst.items()))


def same(a, b):
    """Equal as numbers, element by element (a NaN never is)."""
    return a.shape == b.shape and bool((a.float() == b.float()).all())


def cb8_out(buf, what, c):
    """A CB8 output buffer -> [n][c][h][w] on the CPU, after checking the sentinels and the lanes past c."""
    full = G.from_cb8(buf.cpu(what))
    assert bool((full[:, c:] == 0).all()), f"{what}: lanes past c are not exactly zero"
    return full[:, :c]


class Layer:
    """Device tensors of one (shape, precision): y in CB8, gamma, beta and the statistics of the library's own chain
    (mc_gn_partials with G.TILES tiles -> mc_gn_finalize)."""

    def __init__(self, s, prec):
        L.load()
        self.s, self.prec, self.mc = s, prec, G.MC[prec]
        self.mcg = L.MC_BF16 if self.mc == L.MC_MIX16 else self.mc
        self.ft, self.gt = G.FWD_T[prec], G.GRAD_T[prec]
        y, gamma, beta = G.layer_inputs(s)
        self.y = G.to_cb8(y.to(self.ft)).to(DEV)
        self.gamma, self.beta = gamma.to(DEV), beta.to(DEV)
        self.st = L.stream()
        self.tiles, self.cp = G.tiles_of(s), s.c8 * 8
        self.part = Guarded((s.n, self.tiles, self.cp, 2), torch.float32)
        self.stats = Guarded((s.n, s.groups, 2), torch.float32)
        L.call("mc_gn_partials", L.ptr(self.y), s.n, s.c, s.h, s.w, self.mc, self.tiles, self.part.ptr, self.st)
        L.call("mc_gn_finalize", self.part.ptr, s.n, self.tiles, s.c, s.groups, s.h * s.w, G.EPS, self.stats.ptr, None, self.st)
        self.part.cpu("stat partials")
        self.stats.cpu("stats")

    def dims(self):
        s = self.s
        return s.n, s.c, s.h, s.w

    def source(self, k, src, uploads=None):
        """(mc_grad_src, the device tensor it points into)."""
        s = self.s
        host = G.source_tensor(s, src, k, self.prec)
        uploads = {} if uploads is None else uploads
        if id(host) not in uploads:
            uploads[id(host)] = G.to_cb8(host).to(DEV)
        t = uploads[id(host)]
        return L.GradSrc(L.ptr(t), src.mc_kind, src.pad, 0, src.pool, s.h // src.f, s.w // src.f, src.c8_total, src.cb_off), t


@functools.lru_cache(maxsize=6)
def layer(s, prec):
    return Layer(s, prec)


# ---- statistics ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("prec", G.PRECS)
@pytest.mark.parametrize("s,tiles", G.STAT_CASES, ids=[f"{'x'.join(map(str, s[:5]))}-t{t}{'-8sigma' if s.sigmas else ''}"
                                                       for s, t in G.STAT_CASES])
def test_statistics(s, tiles, prec):
    """mc_gn_partials -> mc_gn_finalize (+ chan_mean) and mc_gn_finalize_coef against f64; the coefficient rows are the f32
    expressions of the emitted statistics bit for bit, rows of padded channels stay untouched."""
    L.load()
    rep = Report(f"statistics {s} tiles {tiles} {prec}")
    mc, st, cp = G.MC[prec], L.stream(), s.c8 * 8
    y, gamma, beta = G.layer_inputs(s)
    y64 = G.stored(y, G.FWD_T[prec])
    yd = G.to_cb8(y.to(G.FWD_T[prec])).to(DEV)
    ptiles = min(tiles, s.h)
    ref = G.stats_ref(y64, s, -(-s.h // ptiles) * s.w)
    part = Guarded((s.n, ptiles, cp, 2), torch.float32)
    L.call("mc_gn_partials", L.ptr(yd), s.n, s.c, s.h, s.w, mc, ptiles, part.ptr, st)
    p = part.cpu("stat partials")
    assert bool((p[:, :, s.c:] == 0).all()), "partials of the padded channels are not zero"
    rep.within("mc_gn_partials", "sum over tiles of the partials", p.double().sum(1)[:, :s.c], ref.sums, ref.dsums)
    if tiles > s.h:                                            # slots of rowless tiles: zeros, as the conv epilogue leaves them
        wide = torch.zeros((s.n, tiles, cp, 2), dtype=torch.float32)
        wide[:, :ptiles] = p
        part = Guarded((s.n, tiles, cp, 2), torch.float32)
        part.t.copy_(wide)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    stats, cmean = Guarded((s.n, s.groups, 2), torch.float32), Guarded((s.n, s.c), torch.float32)
    stats2, coef = Guarded((s.n, s.groups, 2), torch.float32), Guarded((s.n, cp, 4), torch.float32)
    L.call("mc_gn_finalize", part.ptr, s.n, tiles, s.c, s.groups, s.h * s.w, G.EPS, stats.ptr, cmean.ptr, st)
    L.call("mc_gn_finalize_coef", part.ptr, s.n, tiles, s.c, s.groups, s.h * s.w, G.EPS, L.ptr(gd), L.ptr(bd), stats2.ptr,
           coef.ptr, st)
    sg, cm, sg2, cf = stats.cpu("stats"), cmean.cpu("chan_mean"), stats2.cpu("stats (coef)"), coef.cpu("coef4")
    rep.within("mc_gn_finalize", "mean", sg[..., 0], ref.mean, ref.dmean)
    rep.within("mc_gn_finalize", "rstd", sg[..., 1], ref.rstd, ref.rel * ref.rstd)
    hw = s.h * s.w
    rep.within("mc_gn_finalize", "chan_mean", cm, ref.sums[..., 0] / hw, ref.dsums[..., 0] / hw + G.E32 * (ref.sums[..., 0] / hw).abs())
    assert same(sg, sg2), "mc_gn_finalize_coef emits other statistics than mc_gn_finalize"
    mean, rstd = (sg[..., k].repeat_interleave(s.cpg, 1) for k in (0, 1))          # f32 [n][c]
    want = torch.stack([rstd * gamma, beta - mean * rstd * gamma, mean, rstd], -1)
    assert torch.equal(cf[:, :s.c], want), "coef4 is not (rstd g, b - mean rstd g, mean, rstd) of the emitted statistics in f32"
    assert bool(torch.isnan(cf[:, s.c:]).all()), "coef4 rows of padded channels were written"
    rep.show()


# ---- forward ------------------------------------------------------------------------------------------------------------
def run_forward(ly, post, act, pool, with_a=True, y=None, dims=None):
    """mc_gn_act_fwd -> (a [n][c][h][w] or None, pooled or None) on the CPU."""
    n, c, h, w = dims or ly.dims()
    s = ly.s
    gn = post == "gn_act"
    a = Guarded((n, s.c8, h, w, 8), ly.ft) if with_a else None
    pooled = Guarded((n, s.c8, h // pool, w // pool, 8), ly.ft) if pool > 1 else None
    L.call("mc_gn_act_fwd", L.ptr(ly.y if y is None else y), n, c, h, w, s.groups if gn else 0, ly.stats.ptr if gn else None,
           L.ptr(ly.gamma) if gn else None, L.ptr(ly.beta) if gn else None, G.POSTS[post], ACT_ID[act], pool, ly.mc,
           a.ptr if a else None, pooled.ptr if pooled else None, ly.st)
    return (cb8_out(a, "a", c) if a else None), (cb8_out(pooled, "pooled", c) if pooled else None)


def run_forward_small(ly, act, pool):
    """mc_gn_act_fwd_small -> (a, pooled or None, stats)."""
    s = ly.s
    a = Guarded((s.n, s.c8, s.h, s.w, 8), ly.ft)
    pooled = Guarded((s.n, s.c8, s.h // pool, s.w // pool, 8), ly.ft) if pool > 1 else None
    stats = Guarded((s.n, s.groups, 2), torch.float32)
    L.call("mc_gn_act_fwd_small", L.ptr(ly.y), ly.part.ptr, ly.tiles, s.n, s.c, s.h, s.w, s.groups, G.EPS, L.ptr(ly.gamma),
           L.ptr(ly.beta), ACT_ID[act], pool, ly.mc, stats.ptr, a.ptr, pooled.ptr if pooled else None, ly.st)
    return cb8_out(a, "a (one launch)", s.c), (cb8_out(pooled, "pooled (one launch)", s.c) if pooled else None), stats.cpu("stats")


@gpu
@pytest.mark.parametrize("act", G.ACTS)
@pytest.mark.parametrize("prec", G.PRECS)
def test_forward_every_activation_and_post(prec, act):
    s = G.SWEEP
    ly = layer(s, prec)
    rep = Report(f"forward {act} {prec}")
    for post in G.POSTS:
        ref = G.forward_ref(s, prec, post, act, G.addends_of(s))
        a, _ = run_forward(ly, post, act, 1)
        rep.within("mc_gn_act_fwd", f"a, post {post}", a, ref.a, ref.tol)
    rep.show()


@gpu
@pytest.mark.parametrize("act", ("gelu", "selu"))
@pytest.mark.parametrize("prec", G.PRECS)
def test_forward_shapes_and_pooling(prec, act):
    """Two blocks with the grid-stride loop; pool 2 in the row-pair form (16-bit, even W, H >= 2) and in the block form (odd W,
    H = 1, f32); pool 4 with trailing rows and columns; a == NULL.  The pooled tensor is compared with f64 and, in f32, must
    equal mc_avgpool_fwd of the stored a."""
    rep = Report(f"forward shapes {act} {prec}")
    for s, pool, with_a in G.FWD_SHAPES:
        ly = layer(s, prec)
        ref = G.forward_ref(s, prec, "gn_act", act, G.addends_of(s))
        a, pooled = run_forward(ly, "gn_act", act, pool, with_a)
        what = f"{s} pool {pool}" + ("" if with_a else " (a == NULL)")
        if with_a:
            rep.within("mc_gn_act_fwd", "a, " + what, a, ref.a, ref.tol)
        if pool > 1 and s.h < pool:
            assert pooled.numel() == 0                          # (nothing to pool: the sentinels show that nothing was written)
        elif pool > 1:
            pr, pt = G.pooled_ref(ref.a, ref.E, pool, ly.ft)
            assert pooled.shape == pr.shape
            rep.within("mc_gn_act_fwd pooled", "pooled, " + what, pooled, pr, pt)
            if not with_a:
                assert same(pooled, run_forward(ly, "gn_act", act, pool, True)[1]), what + ": pooled depends on a being stored"
            if prec == "f32" and with_a and pooled.numel():
                ad = G.to_cb8(a).to(DEV)
                out = Guarded(tuple(G.to_cb8(pooled).shape), ly.ft)
                L.call("mc_avgpool_fwd", L.ptr(ad), s.n, s.c, s.h, s.w, pool, ly.mc, out.ptr, ly.st)
                assert same(cb8_out(out, "mc_avgpool_fwd", s.c), pooled), what + ": pooled != mc_avgpool_fwd(a)"
    rep.show()


@gpu
@pytest.mark.parametrize("act", ("gelu", "selu"))
@pytest.mark.parametrize("prec", G.PRECS)
def test_forward_one_launch_form(prec, act):
    """mc_gn_act_fwd_small (1, 2, 4, 8 channels per group; c = 12: one group's channel block half empty) at pool 1 and 2: its
    statistics equal mc_gn_finalize's bit for bit, a and the pooled tensor equal mc_gn_act_fwd's (block form: odd W or f32;
    row-pair form: even W in the 16-bit types) and lie within the bound of f64."""
    rep = Report(f"forward one launch {act} {prec}")
    for s in G.SMALL_SHAPES:
        ly = layer(s, prec)
        ref = G.forward_ref(s, prec, "gn_act", act, G.addends_of(s))
        stats0 = ly.stats.cpu("stats")
        for pool in (1, 2):
            a, pooled, stats = run_forward_small(ly, act, pool)
            assert torch.equal(stats, stats0), f"{s}: the one-launch statistics differ from mc_gn_finalize's"
            rep.within("mc_gn_act_fwd_small", f"a, {s} pool {pool}", a, ref.a, ref.tol)
            a0, pooled0 = run_forward(ly, "gn_act", act, pool)
            assert same(a, a0), f"{s} pool {pool}: a differs between the two forms"
            if pool > 1:
                pr, pt = G.pooled_ref(ref.a, ref.E, pool, ly.ft)
                rep.within("mc_gn_act_fwd_small pooled", f"pooled, {s}", pooled, pr, pt)
                assert same(pooled, pooled0), f"{s}: pooled differs between the two forms"
    rep.show()


@gpu
@pytest.mark.parametrize("prec", ("bf16", "mix16"))
def test_pooled_tensor_is_the_same_in_block_and_row_pair_form(prec):
    """The same pixels through both 16-bit forms: a 9 x 13 image takes the block form (odd W); its first 12 columns as an image
    of their own, normalised with the SAME statistics, take the row-pair form.  The six pooled columns must be equal."""
    s = G.Shape(2, 12, 3, 9, 13)
    ly = layer(s, prec)
    _, pooled13 = run_forward(ly, "gn_act", "gelu", 2)
    y12 = ly.y[:, :, :, :12].contiguous()
    a12, pooled12 = run_forward(ly, "gn_act", "gelu", 2, y=y12, dims=(s.n, s.c, s.h, 12))
    a13, _ = run_forward(ly, "gn_act", "gelu", 1)
    assert pooled12.shape == pooled13.shape == (s.n, s.c, 4, 6)
    assert same(pooled12, pooled13) and same(a12, a13[..., :12])


@gpu
@pytest.mark.parametrize("prec", G.PRECS)
def test_avgpool(prec):
    s = G.POOL_SHAPE
    rep = Report(f"avgpool {prec}")
    ft = G.FWD_T[prec]
    x = G.layer_inputs(s)[0].to(ft)
    xd = G.to_cb8(x).to(DEV)
    for f in G.POOL_FACTORS:
        out = Guarded((s.n, s.c8, s.h // f, s.w // f, 8), ft)
        L.call("mc_avgpool_fwd", L.ptr(xd), s.n, s.c, s.h, s.w, f, G.MC[prec], out.ptr, L.stream())
        pr, pt = G.pooled_ref(x.double(), torch.zeros(x.shape, dtype=torch.float64), f, ft)
        rep.within("mc_avgpool_fwd", f"f = {f}", cb8_out(out, "pooled", s.c), pr, pt)
    rep.show()


# ---- backward -----------------------------------------------------------------------------------------------------------
def host_ptrs(*bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])


def run_backward(ly, post, act, srcs, rep, dz_tables=False):
    """Every route the layer can take -- reduce -> finalize -> apply; reduce -> finalize_n + param_grads_batched; the one-launch
    form -- against the reference and, through it, against each other."""
    s, n, c, h, w, cp = ly.s, *ly.dims(), ly.cp
    ref = G.backward_ref(s, ly.prec, post, act, srcs, G.addends_of(s))
    gn = post == "gn_act"
    uploads = {}                                               # slices of one wider tensor point into ONE device tensor
    held = [ly.source(k, src, uploads) for k, src in enumerate(srcs)]
    g0, g1 = C.byref(held[0][0]), (C.byref(held[1][0]) if len(held) > 1 else None)
    tag = f"{s} {post} {act} {'+'.join(x.kind + (str(x.pad) if x.halo else '') + (f'/{x.pool}' if x.f > 1 else '') for x in srcs)}"
    sliced = any(x.c8_total for x in srcs)
    common = (L.ptr(ly.y), n, c, h, w, s.groups if gn else 0, ly.stats.ptr if gn else None)
    gb = (L.ptr(ly.gamma) if gn else None, L.ptr(ly.beta) if gn else None)
    m12 = None
    if gn:
        blocks = L.call("mc_gn_bwd_blocks", h, w)
        part = Guarded((n, blocks, cp, 2), torch.float32)
        L.call("mc_gn_act_bwd_reduce", *common, *gb, G.POSTS[post], ACT_ID[act], ly.mc, g0, g1, part.ptr, ly.st)
        p = part.cpu("reduce partials")
        assert not bool(torch.isnan(p).any()), f"{tag}: a reduce block left its slot unwritten"
        if not sliced:
            assert bool((p[:, :, c:] == 0).all()), f"{tag}: partials of the padded channels are not zero"
        rep.within("mc_gn_act_bwd_reduce", f"partials, {tag}", p.double().sum(1)[:, :c], ref.sums, ref.sums_tol)
        m12 = Guarded((n, s.groups, 2), torch.float32)
        dgamma, dbeta = (Guarded((c,), torch.float32, fill=G.PREFILL) for _ in range(2))
        L.call("mc_gn_act_bwd_finalize", part.ptr, n, blocks, c, s.groups, h * w, L.ptr(ly.gamma), m12.ptr, dgamma.ptr, dbeta.ptr, ly.st)
        rep.within("mc_gn_act_bwd_finalize", f"m12, {tag}", m12.cpu("m12"), ref.m12, ref.m12_tol)
        got = torch.stack([dbeta.cpu("dbeta"), dgamma.cpu("dgamma")])
        rep.within("mc_gn_act_bwd_finalize", f"dbeta / dgamma, {tag}", got, ref.dparam, ref.dparam_tol)
    dy = Guarded((n, s.c8, h, w, 8), ly.gt)
    L.call("mc_gn_act_bwd_apply", *common, m12.ptr if gn else None, *gb, G.POSTS[post], ACT_ID[act], ly.mc, g0, g1, dy.ptr, ly.st)
    rep.within("mc_gn_act_bwd_apply", f"dy, {tag}", cb8_out(dy, "dy", c), ref.dy, ref.dy_tol, ref.keep)
    if not (gn and s.small):
        return
    # the _n finalize on the same partials, and the one-launch form
    m12n, pcn = Guarded((n, s.groups, 2), torch.float32), Guarded((n, cp, 2), torch.float32)
    L.call("mc_gn_act_bwd_finalize_n", part.ptr, n, blocks, c, s.groups, h * w, L.ptr(ly.gamma), m12n.ptr, pcn.ptr, ly.st)
    dys, pcs = Guarded((n, s.c8, h, w, 8), ly.gt), Guarded((n, cp, 2), torch.float32)
    L.call("mc_gn_act_bwd_small", *common, *gb, ACT_ID[act], ly.mc, g0, g1, dys.ptr, pcs.ptr, ly.st)
    dgs = [Guarded((c,), torch.float32, fill=G.PREFILL) for _ in range(4)]
    counts = (C.c_int32 * 2)(n, n), (C.c_int32 * 2)(c, c)
    L.call("mc_gn_param_grads_batched", host_ptrs(pcn, pcs), counts[0], counts[1], host_ptrs(dgs[0], dgs[2]),
           host_ptrs(dgs[1], dgs[3]), 2, ly.st)
    rep.within("mc_gn_act_bwd_finalize_n", f"m12, {tag}", m12n.cpu("m12 (_n)"), ref.m12, ref.m12_tol)
    pn = pcn.cpu("chan_sums (_n)")
    rep.within("mc_gn_act_bwd_finalize_n", f"chan_sums, {tag}", pn[:, :c], ref.sums, ref.sums_tol)
    assert bool(torch.isnan(pn[:, c:]).all()), f"{tag}: finalize_n wrote chan_sums rows of padded channels"
    rep.within("mc_gn_act_bwd_small", f"dy, {tag}", cb8_out(dys, "dy (one launch)", c), ref.dy, ref.dy_tol, ref.keep)
    ps = pcs.cpu("chan_sums (one launch)")
    rep.within("mc_gn_act_bwd_small", f"chan_sums, {tag}", ps[:, :c], ref.sums, ref.sums_tol)
    if not sliced:
        assert bool((ps[:, c:] == 0).all()), f"{tag}: chan_sums of the padded channels are not zero"
    for k, fam in ((0, "mc_gn_act_bwd_finalize_n"), (2, "mc_gn_act_bwd_small")):
        got = torch.stack([dgs[k + 1].cpu("dbeta (batched)"), dgs[k].cpu("dgamma (batched)")])
        rep.within("mc_gn_param_grads_batched", f"dbeta / dgamma after {fam}, {tag}", got, ref.dparam, ref.dparam_tol)


@gpu
@pytest.mark.parametrize("act", G.ACTS)
@pytest.mark.parametrize("prec", G.PRECS)
def test_backward_every_activation_and_post(prec, act):
    ly = layer(G.SWEEP, prec)
    rep = Report(f"backward {act} {prec}")
    for post in G.POSTS:
        run_backward(ly, post, act, G.SRC_SWEEP, rep)
    rep.show()


@gpu
@pytest.mark.parametrize("prec,act", [("bf16", "gelu"), ("bf16", "selu"), ("mix16", "gelu"), ("mix16", "selu"), ("f32", "selu")])
def test_backward_every_source_kind(prec, act):
    """The compile-time kinds GK = 2, 1, 3 of the 16-bit types and the run-time path (pooled sources with floor mode and
    1 / f^2, slices of a wider tensor), each on both routes."""
    rep = Report(f"backward sources {act} {prec}")
    for s, srcs in G.SOURCE_CASES:
        run_backward(layer(s, prec), "gn_act", act, srcs, rep)
    rep.show()


@gpu
@pytest.mark.parametrize("prec", G.PRECS)
@pytest.mark.parametrize("s", G.LAUNCH_SHAPES, ids=["x".join(map(str, s[:5])) for s in G.LAUNCH_SHAPES])
def test_backward_launch_shape_edges(s, prec):
    """32 / 16 / 8 rows per apply block with a ragged last block; a reduction whose blocks take different numbers of rows, and
    one with a rowless block, which must write zeros."""
    rep = Report(f"backward launch shapes {s} {prec}")
    run_backward(layer(s, prec), "gn_act", "gelu", (G.Src("plain"),), rep)
    rep.show()


@gpu
@pytest.mark.parametrize("prec", G.PRECS)
def test_backward_general_group_width(prec):
    """3 and 16 channels per group: the general path of k_gn_bwd_finalize (no one-launch form)."""
    rep = Report(f"backward general groups {prec}")
    for s in G.GENERAL_SHAPES:
        run_backward(layer(s, prec), "gn_act", "selu", G.SRC_SWEEP, rep)
    rep.show()


@gpu
@pytest.mark.parametrize("blocks", G.CHUNK_BLOCKS)
def test_finalize_across_the_sample_chunk(blocks):
    """257 samples (256 per LDS round) from host-made partials with 1, 3 and 5 slots: mc_gn_act_bwd_finalize, and
    mc_gn_act_bwd_finalize_n (four waves, some without a slot) + mc_gn_param_grads_batched."""
    L.load()
    s, st = G.CHUNK_SHAPE, L.stream()
    rep = Report(f"finalize N = {s.n} blocks {blocks}")
    part, gamma = G.chunk_partials(blocks)
    m12r, m12t, dpr, dpt, sums, sums_t = G.finalize_ref(part, gamma, s)
    pd, gd = part.to(DEV), gamma.to(DEV)
    m12, m12n, pc = Guarded((s.n, s.groups, 2), torch.float32), Guarded((s.n, s.groups, 2), torch.float32), Guarded((s.n, 8, 2), torch.float32)
    dg = [Guarded((s.c,), torch.float32, fill=G.PREFILL) for _ in range(4)]
    L.call("mc_gn_act_bwd_finalize", L.ptr(pd), s.n, blocks, s.c, s.groups, s.h * s.w, L.ptr(gd), m12.ptr, dg[0].ptr, dg[1].ptr, st)
    L.call("mc_gn_act_bwd_finalize_n", L.ptr(pd), s.n, blocks, s.c, s.groups, s.h * s.w, L.ptr(gd), m12n.ptr, pc.ptr, st)
    L.call("mc_gn_param_grads_batched", host_ptrs(pc), (C.c_int32 * 1)(s.n), (C.c_int32 * 1)(s.c), host_ptrs(dg[2]), host_ptrs(dg[3]), 1, st)
    rep.within("mc_gn_act_bwd_finalize", "m12", m12.cpu("m12"), m12r, m12t)
    rep.within("mc_gn_act_bwd_finalize_n", "m12", m12n.cpu("m12 (_n)"), m12r, m12t)
    rep.within("mc_gn_act_bwd_finalize_n", "chan_sums", pc.cpu("chan_sums"), sums, sums_t)
    rep.within("mc_gn_act_bwd_finalize", "dbeta / dgamma", torch.stack([dg[1].cpu("dbeta"), dg[0].cpu("dgamma")]), dpr, dpt)
    rep.within("mc_gn_param_grads_batched", "dbeta / dgamma", torch.stack([dg[3].cpu("dbeta"), dg[2].cpu("dgamma")]), dpr, dpt)
    rep.show()


@gpu
@pytest.mark.parametrize("s", [G.SWEEP, G.GENERAL_SHAPES[0]], ids=["4-per-group", "3-per-group"])
def test_finalize_dz_tables(s):
    """The _dz finalize forms: m12 as the plain forms give it, and dz_coef rows (cA, cB, cC, mean) = (scale, -rstd^2 m2,
    -rstd m1, mean) evaluated in f32 from coef and the emitted m12, bit for bit; rows of padded channels stay untouched."""
    ly = layer(s, "f32")
    n, c, h, w, cp, st = *ly.dims(), ly.cp, ly.st
    rep = Report(f"finalize _dz {s}")
    ref = G.backward_ref(s, "f32", "gn_act", "gelu", (G.Src("plain"),), G.addends_of(s))
    coef = Guarded((n, cp, 4), torch.float32, fill=0.0)
    L.call("mc_gn_finalize_coef", ly.part.ptr, n, ly.tiles, c, s.groups, h * w, G.EPS, L.ptr(ly.gamma), L.ptr(ly.beta), None, coef.ptr, st)
    src, keep = ly.source(0, G.Src("plain"))
    blocks = L.call("mc_gn_bwd_blocks", h, w)
    part = Guarded((n, blocks, cp, 2), torch.float32)
    L.call("mc_gn_act_bwd_reduce", L.ptr(ly.y), n, c, h, w, s.groups, ly.stats.ptr, L.ptr(ly.gamma), L.ptr(ly.beta), L.POST_GN_ACT,
           ACT_ID["gelu"], ly.mc, C.byref(src), None, part.ptr, st)
    m12 = Guarded((n, s.groups, 2), torch.float32)
    L.call("mc_gn_act_bwd_finalize", part.ptr, n, blocks, c, s.groups, h * w, L.ptr(ly.gamma), m12.ptr, None, None, st)
    want_m12, cf = m12.cpu("m12"), coef.cpu("coef4")
    forms = [("mc_gn_act_bwd_finalize_dz", False)] + ([("mc_gn_act_bwd_finalize_n_dz", True)] if s.small else [])
    for name, per_sample in forms:
        m, dzc = Guarded((n, s.groups, 2), torch.float32), Guarded((n, cp, 4), torch.float32)
        if per_sample:
            pc = Guarded((n, cp, 2), torch.float32)
            L.call(name, part.ptr, n, blocks, c, s.groups, h * w, L.ptr(ly.gamma), m.ptr, pc.ptr, coef.ptr, dzc.ptr, st)
            pc.cpu("chan_sums")
        else:
            dg, db = (Guarded((c,), torch.float32, fill=G.PREFILL) for _ in range(2))
            L.call(name, part.ptr, n, blocks, c, s.groups, h * w, L.ptr(ly.gamma), m.ptr, dg.ptr, db.ptr, coef.ptr, dzc.ptr, st)
            dg.cpu("dgamma"), db.cpu("dbeta")
        got_m, got = m.cpu("m12"), dzc.cpu("dz_coef")
        if not per_sample:
            assert torch.equal(got_m, want_m12), f"{name}: m12 differs from mc_gn_act_bwd_finalize's"
        rep.within(name, "m12", got_m, ref.m12, ref.m12_tol)
        m1, m2 = (got_m[..., k].repeat_interleave(s.cpg, 1) for k in (0, 1))        # f32 [n][c]
        sc, mean, rstd = cf[:, :c, 0], cf[:, :c, 2], cf[:, :c, 3]
        want = torch.stack([sc, (-rstd * rstd) * m2, (-rstd) * m1, mean], -1)
        assert torch.equal(got[:, :c], want), f"{name}: dz_coef is not the header's formulas in f32"
        assert bool(torch.isnan(got[:, c:]).all()), f"{name}: dz_coef rows of padded channels were written"
    del keep
    rep.show()

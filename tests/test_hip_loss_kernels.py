"""The Stokes loss kernels of csrc/loss.hip and the curl head of csrc/curl_head.hip against f64, term by term and straight through
the C ABI, at the shapes that cross every kernel's tile seams (tests/loss_cases.py: the case tables, the f64 references, the
derived bounds, the comparison functions; tests/test_loss_cases_host.py puts the mutants through the same comparisons).

  A  mc_momentum_adjoint as a linear operator: random S, eta in (1e-8, 1], every pixel of all four planes, ra = 2.5, inv_h = 63
  B  mc_momentum_residual: eta_ws, the exact signs outside a per-pixel kink bound, the exactly-zero ring, the two sums, p = NULL
  C  the momentum term alone in mc_loss_fused (lambda = 1, truth = prediction bit for bit), plane and CB8 forms, and bit-equal to
     mc_loss_fwd_bwd + mc_momentum_residual + mc_momentum_adjoint
  D  mc_loss_minmax -> mc_loss_fwd_bwd / mc_loss_fused -> mc_loss_finalize over a covering table of the flags; out8; gsum_part
  E  mc_loss_minmax, mc_loss_finalize, mc_curl_head_fwd / mc_curl_head_bwd on their own

Every buffer a launch writes lies between sentinel bands; buffers written with `=` are prefilled with NaN, buffers written with `+=`
with a known random field g0 (the assertion is on out - g0); the gradient tensors have five channels for a loss that reads three or
four, and the unused channel and every plane a launch must not touch come back bit-identical; the pressure plane and its gradient
have a batch stride of their own in every second case.

Every test prints its worst err / bound (`pytest -s`).  On MI355X, worst over all cases:
  mc_momentum_adjoint      gu, gv, gp, gT 0.83 (the accumulate's own rounding of g0 + x, where x is small against g0)
  mc_momentum_residual     eta_ws 0.49; S exact outside the kink bound (at most 0.02 % of a case left out); sums 0.006
  mc_loss_fused, momentum  gradient 0.34 (at most 0.14 % of a case left out); out8 0.055; bit-equal to the three kernels, both forms
  mc_loss_fwd_bwd          gradient 0.33; out8 0.043
  mc_loss_fused            gradient 0.16; out8 0.064; gsum_part 0.060, two runs bit-identical
  mc_loss_minmax           exact;  mc_loss_finalize 0.85 (the bound is the one rounding to f32)
  mc_curl_head_fwd / bwd   u, v 0.33 (one rounding of the three allowed); ga 0.25; clip and its gradient exact; adjoint identity 0.006
With `gp += dP` of k_loss_fused and the gp_ line of k_mom_adjoint commented out, parts A and C fail on the gp plane (run once)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import loss_cases as Lc
from pbml_mantle_convection_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7B
f32, f64 = torch.float32, torch.float64
NAN = float("nan")
ALL = [(Lc.B, H, W) for H, W in Lc.SHAPES]


class Guarded:
    """A tensor between two sentinel bands inside one larger allocation (restated from tests/test_hip_gn_act.py)."""

    def __init__(self, shape, dtype=f32, fill=NAN, guard_bytes=65536):
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.to(dtype))
        elif fill is not None:
            self.t.fill_(fill)
        self.before = self.t.clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.g

    def cpu(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[:self.g] == SENTINEL).all()), f"{what}: bytes BEFORE the buffer were overwritten"
        assert bool((self.raw[self.g + self.nbytes:] == SENTINEL).all()), f"{what}: bytes BEHIND the buffer were overwritten"
        return self.t.cpu()

    def untouched(self, what, index):
        """The slice comes back bit-identical to what it held before the launch."""
        a, b = self.t[index].contiguous(), self.before[index].contiguous()
        assert torch.equal(a.view(torch.int32) if a.dtype == f32 else a.view(torch.int64),
                           b.view(torch.int32) if b.dtype == f32 else b.view(torch.int64)), f"{what} was written"


def dev(t):
    return t.to(f32).to(DEV).contiguous()


def desc(N, H, W, p_pred=True, loss_type=0, ls=False, ld=False, l2=False, lam=0.0, t_grad=1, ra=Lc.RA, ih=Lc.INV_H):
    return L.LossDesc(N, H, W, int(p_pred), loss_type, int(ls), int(ld), int(l2), lam, ih, ra, t_grad)


def garbage(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=f64) * 3.0e4


class Planes:
    """A five-channel tensor [N, 5, H, W] holding the planes u, v, T, p in channels 0..3 (channel 4 is not the loss's), and, when
    `split`, the p plane in channel 0 of a two-channel tensor of its own (ppbs = 2 HW != pbs = 5 HW)."""

    def __init__(self, N, H, W, split, fill):
        self.N, self.HW, self.split = N, H * W, split
        self.y = Guarded((N, 5, H, W), fill=fill)
        self.q = Guarded((N, 2, H, W), fill=fill[:, 3:5] if isinstance(fill, torch.Tensor) else fill) if split else None
        self.pbs, self.ppbs = 5 * H * W, (2 if split else 5) * H * W

    def ptr(self, ch):
        if ch == 3 and self.split:
            return self.q.ptr
        return self.y.ptr + 4 * ch * self.HW

    def planes(self, what):
        y = self.y.cpu(what).double()
        out = [y[:, 0], y[:, 1], y[:, 2], y[:, 3]]
        if self.split:
            out[3] = self.q.cpu(what + " (p)").double()[:, 0]
        return out

    def check_untouched(self, what, written):
        """`written`: the channels of (u, v, T, p) the launch may write."""
        for ch in range(5):
            if ch == 4 or ch not in written or (ch == 3 and self.split):
                self.y.untouched(f"{what}: channel {ch} of the five", (slice(None), ch))
        if self.split:
            self.q.untouched(f"{what}: the gap behind the p plane", (slice(None), 1))
            if 3 not in written:
                self.q.untouched(f"{what}: the p plane", (slice(None), 0))


def pred_planes(d, split, seed=1):
    N, H, W = d["u"].shape
    fill = garbage((N, 5, H, W), seed)
    for ch, k in enumerate(("u", "v", "T", "p")):
        fill[:, ch] = d[k]
    return Planes(N, H, W, split, fill)


def report(tag, **worst):
    print(f"\n[{tag}] worst err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- A: the momentum adjoint as a linear operator -------------------------------------------------------------------------
A_CASES = [(N, H, W, 1, True, i % 2 == 1) for i, (N, H, W) in enumerate(ALL)] + [
    (Lc.B, 9, 66, 0, True, False),        # T given: the gT plane is not touched
    (Lc.B, 9, 66, 1, False, True),        # gp = NULL
    (Lc.B, 17, 65, 0, False, False)]


@pytest.mark.parametrize("N,H,W,t_grad,with_p,split", A_CASES)
def test_momentum_adjoint_is_the_transpose_of_the_residual(N, H, W, t_grad, with_p, split):
    c = Lc.adjoint_case(N, H, W)
    g0 = c["g0"]
    out = Planes(N, H, W, split, g0)
    sx, sy, eta, s = dev(c["sx"]), dev(c["sy"]), dev(c["eta"]), dev(c["s"])
    dummy = torch.zeros(4, device=DEV)
    d = desc(N, H, W, lam=1.0, t_grad=t_grad)
    L.call("mc_momentum_adjoint", C.byref(d), L.ptr(dummy), out.pbs, out.ppbs, L.ptr(eta), L.ptr(dummy), L.ptr(s), L.ptr(sx), L.ptr(sy),
           out.ptr(0), out.ptr(1), out.ptr(3) if with_p else None, out.ptr(2), L.stream())
    got = out.planes("gradient planes")
    written = {0, 1} | ({3} if with_p else set()) | ({2} if t_grad else set())
    out.check_untouched("mc_momentum_adjoint", written)
    ref = dict(zip((0, 1, 3, 2), c["ref"]))               # adjoint64 orders (u, v, p, T); the channels are (u, v, T, p)
    tol = dict(zip((0, 1, 3, 2), c["tol"]))
    chs = sorted(written)
    fails, worst = Lc.check_planes([Lc.PLANES[ch] for ch in chs], [got[ch] - g0[:, ch] for ch in chs], [ref[ch] for ch in chs],
                                   [tol[ch] for ch in chs])
    report("A mc_momentum_adjoint", planes=worst)
    assert not fails, fails


# ---- B: the momentum residual ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def residual_ref(N, H, W, p_null=False):
    return Lc.Residual(Lc.inputs(N, H, W), 1e-6, p_null=p_null)


@pytest.mark.parametrize("N,H,W,p_null,split", [(N, H, W, False, i % 2 == 0) for i, (N, H, W) in enumerate(ALL + [Lc.MANY])]
                         + [(Lc.B, 9, 66, True, False)])
def test_momentum_residual(N, H, W, p_null, split):
    d_in = Lc.inputs(N, H, W)
    r = residual_ref(N, H, W, p_null)
    y = pred_planes(d_in, split)
    sx, sy, eta = (Guarded((N, H, W)) for _ in range(3))
    sums = Guarded((L.LOSS_SLOTS,), f64, 0.0)
    yc, paras, s = dev(d_in["yc"]), dev(d_in["paras"]), dev(d_in["scaler"])
    d = desc(N, H, W, lam=1e-6)
    L.call("mc_momentum_residual", C.byref(d), y.ptr(0), y.ptr(1), None if p_null else y.ptr(3), y.ptr(2), y.pbs, y.ppbs, L.ptr(yc),
           L.ptr(paras), L.ptr(s), sums.ptr, sx.ptr, sy.ptr, eta.ptr, L.stream())
    sm = sums.cpu("sums")
    assert bool((sm[:13] == 0).all()) and float(sm[15]) == 0.0
    fails, worst = Lc.check_residual(r, sx.cpu("sx").double(), sy.cpu("sy").double(), eta.cpu("eta_ws").double(), (sm[13], sm[14]))
    report("B mc_momentum_residual", **worst)
    assert not fails, fails


def test_many_samples_case_walks_more_than_one_tile_per_block():
    """The launch formulas restated in loss_cases.py are the kernels' (mc_loss_fused_blocks is the one the library exposes), and at
    N = 256, 33 x 129 each of the three loop kernels has fewer blocks per sample than tiles."""
    N, H, W = Lc.MANY
    for n, h, w in ALL + [Lc.MANY, (1, 128, 506), (32, 128, 506)]:
        assert L.call("mc_loss_fused_blocks", n, h, w) == Lc.grid_fused(n, h, w)
    assert Lc.cdiv(1024, N) < Lc.tiles(H, W, Lc.LT_TH) == 6 and Lc.grid_loss(N, H, W) < 6
    assert L.call("mc_loss_fused_blocks", N, H, W) < Lc.tiles(H, W, Lc.LF_TH) == 15 and Lc.cdiv(2048, N) < 15
    assert 2 * Lc.cdiv(1024, N) < Lc.tiles(H, W, Lc.MR_TH) == 9 and Lc.grid_residual(N, H, W) < 9


# ---- C, D: the gradient kernels ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_ref(N, H, W, route, p_pred, loss_type, ls, ld, l2, t_grad, lam, self_truth):
    d = Lc.inputs(N, H, W)
    truth = torch.stack([d["u"], d["v"], d["p"], d["T"]], 1) if self_truth else None
    th, grid = (Lc.LF_TH, Lc.grid_fused(N, H, W)) if route == "fused" else (Lc.LT_TH, Lc.grid_loss(N, H, W))
    return Lc.StokesGrad(d, truth=truth, p_pred=p_pred, loss_type=loss_type, ls=ls, ld=ld, l2=l2, t_grad=t_grad, lam=lam,
                         thread_adds=Lc.adds_per_thread(N, H, W, th, grid))


class Run:
    """One evaluation of the loss through the C ABI: mc_loss_minmax (with loss_scale), the gradient kernels of `route`, then
    mc_loss_finalize."""

    def __init__(self, g, N, H, W, route, p_pred, loss_type, ls, ld, l2, t_grad, lam, split, gsum=False):
        d_in = Lc.inputs(N, H, W)
        has_T = t_grad >= 0
        self.out = Planes(N, H, W, split, NAN)
        y = pred_planes(d_in, split)
        uvp = dev(g.truth)
        ct = uvp.shape[1]
        self.mm = Guarded((N, 3, 2))
        sums, self.out8 = Guarded((L.LOSS_SLOTS,), f64, 0.0), Guarded((8,))
        d = desc(N, H, W, p_pred, loss_type, ls, ld, l2, lam, t_grad)
        st = L.stream()
        if ls:
            L.call("mc_loss_minmax", L.ptr(uvp), N, ct, H, W, self.mm.ptr, st)
        mom = lam != 0.0
        yc, paras, s = (dev(d_in[k]) if mom else None for k in ("yc", "paras", "scaler"))
        o, P = self.out, (lambda ch, ok=True: y.ptr(ch) if ok else None)
        self.gsum = None
        if route == "three":
            L.call("mc_loss_fwd_bwd", C.byref(d), P(0), P(1), P(3, p_pred), P(2, has_T), y.pbs, y.ppbs, L.ptr(uvp), self.mm.ptr, sums.ptr,
                   o.ptr(0), o.ptr(1), o.ptr(3) if p_pred else None, o.ptr(2) if has_T else None, st)
            if mom:
                sx, sy, eta = (Guarded((N, H, W)) for _ in range(3))
                L.call("mc_momentum_residual", C.byref(d), P(0), P(1), P(3, p_pred), P(2), y.pbs, y.ppbs, L.ptr(yc), L.ptr(paras), L.ptr(s),
                       sums.ptr, sx.ptr, sy.ptr, eta.ptr, st)
                L.call("mc_momentum_adjoint", C.byref(d), P(2), y.pbs, y.ppbs, eta.ptr, L.ptr(paras), L.ptr(s), sx.ptr, sy.ptr,
                       o.ptr(0), o.ptr(1), o.ptr(3) if p_pred else None, o.ptr(2), st)
                sx.cpu("sx"), sy.cpu("sy"), eta.cpu("eta_ws")
        else:
            if gsum:
                self.blocks = int(L.call("mc_loss_fused_blocks", N, H, W))
                self.gsum = Guarded((N, self.blocks, 4))
            tail = (L.ptr(uvp), self.mm.ptr, L.ptr(yc), L.ptr(paras), L.ptr(s), sums.ptr, o.ptr(0), o.ptr(1), o.ptr(3) if p_pred else None,
                    o.ptr(2), o.pbs, o.ppbs, self.gsum.ptr if gsum else None, st)
            if route == "cb8":
                crop = 3
                buf = garbage((N, 1, H, W + 2 * crop, 8), 11)                     # crop columns and lanes 4..7: garbage
                buf[:, 0, :, crop:crop + W, :4] = torch.stack([d_in[k] for k in ("u", "v", "T", "p")], -1)
                self.buf, self.mean = dev(buf), torch.zeros((N, 5), device=DEV)
                L.call("mc_loss_fused", C.byref(d), None, None, None, None, 0, 0, L.ptr(self.buf), W + 2 * crop, crop, L.ptr(self.mean), 5, *tail)
            else:
                L.call("mc_loss_fused", C.byref(d), P(0), P(1), P(3, p_pred), P(2), y.pbs, y.ppbs, None, 0, 0, None, 0, *tail)
        L.call("mc_loss_finalize", C.byref(d), sums.ptr, self.out8.ptr, st)
        self.written = {0, 1} | ({3} if p_pred else set()) | ({2} if has_T else set())
        self.planes = self.out.planes(route + " gradient planes")
        self.out.check_untouched(route, self.written)
        y.check_untouched(route + " (inputs)", set())
        sums.cpu("sums")
        self.o8 = self.out8.cpu("out8").double()
        if not ls or ct == 2:
            self.mm.cpu("mm")
            self.mm.untouched("mm", (slice(None), 2) if ls else slice(None))

    def check(self, g, tag):
        chs = sorted(self.written)
        fails, worst = Lc.check_planes([Lc.PLANES[c] for c in chs], [self.planes[c] for c in chs], [g.grad[c] for c in chs],
                                       [g.tol[c] for c in chs], [g.keep[c] for c in chs])
        f2, w2 = Lc.check_scalars(Lc.OUT_NAMES, self.o8, g.out, g.out_tol)
        report(tag, gradient=worst, out8=w2)
        assert not fails + f2, fails + f2


@pytest.mark.parametrize("N,H,W,split", [(N, H, W, i % 2 == 0) for i, (N, H, W) in enumerate(ALL + [Lc.MANY])])
def test_momentum_term_alone_in_the_one_launch_kernel(N, H, W, split):
    """lambda = 1, loss_type 0, no derivative, truth = prediction bit for bit: every data-term gradient is exactly zero, and the
    output is the momentum adjoint and nothing else."""
    flags = (True, 0, False, False, False, 1, 1.0)
    g = grad_ref(N, H, W, "fused", *flags, True)
    runs = {route: Run(g, N, H, W, route, *flags, split) for route in ("fused", "cb8", "three")}
    runs["fused"].check(g, "C mc_loss_fused, planes")
    runs["cb8"].check(g, "C mc_loss_fused, CB8")
    for route in ("cb8", "three"):
        for a, b, n in zip(runs["fused"].planes, runs[route].planes, Lc.PLANES):
            assert torch.equal(a, b), (route, n, float((a - b).abs().max()))


D_CASES = [(N, H, W) + fc for (N, H, W) in ALL for fc in Lc.FLAG_CASES] + [Lc.MANY + Lc.FLAG_CASES[1], Lc.MANY + Lc.FLAG_CASES[5]]


@pytest.mark.parametrize("N,H,W,route,p_pred,loss_type,ls,ld,l2,t_grad", D_CASES)
def test_data_derivative_and_mass_terms(N, H, W, route, p_pred, loss_type, ls, ld, l2, t_grad):
    route = "three" if route == "fwd_bwd" else route
    flags = (p_pred, loss_type, ls, ld, l2, t_grad, 0.0)
    g = grad_ref(N, H, W, route, *flags, False)
    split = (H + loss_type + int(ls)) % 2 == 0
    fused = route == "fused"
    r = Run(g, N, H, W, route, *flags, split, gsum=fused)
    r.check(g, f"D {route}")
    if ls:                                                             # mc_loss_minmax inside the route: exact
        mm = r.mm.cpu("mm").double()
        ct = g.truth.shape[1]
        for f in range(min(ct, 3)):
            assert torch.equal(mm[:, f, 0], g.truth[:, f].amin((1, 2))) and torch.equal(mm[:, f, 1], g.truth[:, f].amax((1, 2)))
    if fused:
        # D5: the per-block sums of the gradient planes, finalised, are the spatial sums of the planes the kernel wrote
        part = r.gsum.cpu("gsum_part")
        scale = 0.5
        out = Guarded((N, 4))
        L.call("mc_partial_sums_finalize", r.gsum.ptr, N, r.blocks, 4, scale, out.ptr, L.stream())
        got = out.cpu("gradient sums").double()
        ref = torch.stack([scale * p.sum((1, 2)) for p in r.planes], 1)
        if not p_pred:
            ref[:, 3] = 0.0
            assert bool((got[:, 3] == 0).all())
        # a thread's running sum, six wave levels, four waves, the blocks in order, the scale
        depth = Lc.adds_per_thread(N, H, W, Lc.LF_TH, r.blocks) + 6 + 3 + r.blocks + 1
        tol = torch.stack([depth * Lc.U * scale * p.abs().sum((1, 2)) for p in r.planes], 1)
        if not p_pred:
            tol[:, 3] = 0.0
        w, bad = Lc.compare(got, ref, tol)
        report("D gsum_part", sums=w)
        assert not bool(bad.any()), (got, ref)
        r2 = Run(g, N, H, W, route, *flags, split, gsum=True)
        assert torch.equal(r2.gsum.cpu("gsum_part"), part)
        for ch in sorted(r.written):
            assert torch.equal(r.planes[ch], r2.planes[ch]), Lc.PLANES[ch]


# ---- E: the small kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,ct,kind", [(3, 7, 3, "random"), (1, 263, 4, "random"), (19, 27, 3, "negative"), (19, 27, 2, "last"),
                                         (5, 5, 2, "negative"), (33, 129, 4, "last")])
def test_loss_minmax(H, W, ct, kind):
    """hw < 256, a prime hw, hw = 256 k + 1 (19 x 27 = 513); all-negative fields; the extremum in the last element; with two
    channels the third row of mm is not touched."""
    N = 3
    g = torch.Generator().manual_seed(H * W + ct)
    x = Lc.r32(torch.randn((N, ct, H, W), generator=g, dtype=f64))
    if kind == "negative":
        x = Lc.r32(-x.abs() - 0.5)
    if kind == "last":
        x[:, 0, -1, -1] = 9.0
        x[:, 1, -1, -1] = -9.0
    mm = Guarded((N, 3, 2))
    L.call("mc_loss_minmax", L.ptr(dev(x)), N, ct, H, W, mm.ptr, L.stream())
    got = mm.cpu("mm").double()
    for f in range(min(ct, 3)):
        assert torch.equal(got[:, f, 0], x[:, f].amin((1, 2))) and torch.equal(got[:, f, 1], x[:, f].amax((1, 2))), f
    if ct == 2:
        mm.untouched("the third row of mm", (slice(None), 2))


def test_loss_finalize_formulas():
    """Synthetic f64 sums through every combination of loss_type, p_pred, loss_scale, loss_derivative, t_grad and lambda."""
    N, H, W = 3, 9, 66
    sums = torch.rand(L.LOSS_SLOTS, generator=torch.Generator().manual_seed(5), dtype=f64) * 100.0 + 1.0
    sd = sums.to(DEV)
    combos = [(lt, pp, ls, ld, tg, lam) for lt in (0, 1, 2) for pp in (0, 1) for ls in (0, 1) for ld in (0, 1) for tg in (-1, 0, 1)
              for lam in (0.0, 1e-6)]
    out = Guarded((len(combos), 8))
    for i, (lt, pp, ls, ld, tg, lam) in enumerate(combos):
        d = desc(N, H, W, pp, lt, ls, ld, False, lam, tg)
        L.call("mc_loss_finalize", C.byref(d), L.ptr(sd), out.ptr + 32 * i, L.stream())
    got = out.cpu("out8").double()
    worst = 0.0
    for i, (lt, pp, ls, ld, tg, lam) in enumerate(combos):
        ref = Lc.finalize64(sums, N, H, W, pp, lt, ls, ld, tg, lam)
        # f64 arithmetic (a dozen operations of 2^-53) and one rounding to f32
        f, w = Lc.check_scalars(Lc.OUT_NAMES, got[i], ref, [Lc.U * abs(r) + 16 * 2.0 ** -53 * abs(r) for r in ref])
        worst = max(worst, w)
        assert not f, (combos[i], f)
    report("E mc_loss_finalize", out8=worst)


@pytest.mark.parametrize("H,W", Lc.CURL_SHAPES)
@pytest.mark.parametrize("with_t", [True, False])
def test_curl_head(H, W, with_t):
    c = Lc.curl_case(H, W)
    N = c["a"].shape[0]
    HW = H * W
    yin = garbage((N, 3, H, W), 21)                                    # batch stride 3 HW: a, t, a gap
    yin[:, 0], yin[:, 1] = c["a"], c["t"]
    y = Guarded((N, 3, H, W), fill=yin)
    u, v, tc = (Guarded((N, H, W)) for _ in range(3))
    st = L.stream()
    L.call("mc_curl_head_fwd", y.ptr, y.ptr + 4 * HW if with_t else None, N, H, W, 3 * HW, Lc.A_BOUND, Lc.T_LO, Lc.T_HI, u.ptr, v.ptr,
           tc.ptr if with_t else None, st)
    uk, vk = u.cpu("u").double(), v.cpu("v").double()
    y.untouched("the input", slice(None))
    fails, w_uv = Lc.check_planes(["u", "v"], [uk, vk], [c["u"], c["v"]], [c["u_tol"], c["v_tol"]])
    for t in (uk, vk):
        for i in (0, -1):
            for j in (0, -1):
                assert bool((t[:, i, j] == 0).all()), "corners come out exactly 0"
    if with_t:
        assert torch.equal(tc.cpu("t_out").double(), c["tc"])
    else:
        tc.untouched("t_out", slice(None))
    gu, gv, gt = dev(c["gu"]), dev(c["gv"]), dev(c["gt"])
    gy = Guarded((N, 3, H, W))
    ws = Guarded((2 * N * (H - 2) * (W - 2),))
    L.call("mc_curl_head_bwd", L.ptr(gu), L.ptr(gv), L.ptr(gt) if with_t else None, y.ptr + 4 * HW if with_t else None, N, H, W,
           Lc.A_BOUND, Lc.T_LO, Lc.T_HI, gy.ptr, gy.ptr + 4 * HW if with_t else None, 3 * HW, 3 * HW, ws.ptr, st)
    g = gy.cpu("ga").double()
    ws.cpu("workspace")
    f2, w_ga = Lc.check_planes(["ga"], [g[:, 0]], [c["ga"]], [c["ga_tol"]])      # (NaN prefill: every pixel of ga is written)
    gy.untouched("the gap behind the gradient planes", (slice(None), 2))
    if with_t:
        assert torch.equal(g[:, 1], c["gt_in"]), "the clip passes the gradient where t_lo <= t <= t_hi, the bounds included"
    else:
        gy.untouched("the t plane of the gradient", (slice(None), 1))
    # <curl(a), g> = <a, curl^T g> in f64 of the kernels' outputs
    lhs = float((uk * c["gu"]).sum() + (vk * c["gv"]).sum())
    rhs = float((c["a"] * g[:, 0]).sum())
    tol = float((c["gu"].abs() * c["u_tol"]).sum() + (c["gv"].abs() * c["v_tol"]).sum() + (c["a"].abs() * c["ga_tol"]).sum())
    report("E curl head", uv=w_uv, ga=w_ga, adjoint=abs(lhs - rhs) / tol)
    assert not fails + f2, fails + f2
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)

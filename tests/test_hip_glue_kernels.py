"""The kernels that carry every tensor between the convolutions, path by path against f64 and straight through the C ABI: the
NCHW <-> CB8 converters and mc_sum_hw, mc_rect_copy, mc_gsrc_sum, the padding adjoint (mc_fold_padded, mc_fold_padded2,
mc_fold_padded_dz) of csrc/layout.hip and csrc/groupnorm.hip and the six bicubic entry points of csrc/bicubic.hip.  tests/glue_cases.py holds the case tables, the f64
references, the bounds derived from the kernels' rounding counts and the comparison functions; tests/test_glue_cases_host.py puts
the mutants through the same comparisons and checks the launch arithmetic that makes each case reach its path.

Every buffer a launch writes lies between sentinel bands and is prefilled with NaN (in-place kernels: with their input, and what
they must not touch comes back bit for bit); gradient sources carry NaN in their halo and in the channel blocks of a wider tensor
that are not theirs.

Every test prints its worst err / bound (`pytest -s`); the last test prints the table per family.  On MI355X, worst over all
cases (f32 stores | 16-bit stores, where the bound is the store's own rounding and a correct kernel comes close to it):
  mc_pack_nchw, mc_unpack_nchw, mc_pack_grad_nchw, mc_rect_copy   exact, every case
  mc_sum_hw                            0.019 (hw = 1: the product with the scale, one rounding of the 22 allowed)
  mc_sum_hw -> mc_pack_grad_nchw       0.96 (the 16-bit store; the difference's one rounding in f32)
  mc_gsrc_sum                          0.998 | 0.996 (f32: g0 + g1 is ONE rounding and the bound is one rounding)
  mc_fold_padded, mc_fold_padded2      1.00 | 0.996 (f32: a pixel with two sources is one rounding, the bound is one); two buffers
                                       bit-equal to two single calls
  mc_fold_padded_dz                    dz 0.58 | 0.996; partials 0.14 | 0.25; no kink pixel in any case
  bicubic forward, tiled / direct      0.26 | 0.99
  bicubic forward, walk                0.30 | 0.997
  bicubic forward with GELU            0.18 | 0.85
  bicubic adjoint, walk                0.13 | 0.995
  bicubic adjoint, taps                0.050 | 0.994
  bicubic adjoint, separable           0.048 | 0.96
No derived bound was exceeded and no kernel was changed.  With the cb_off term of k_bicubic_bwd_walk removed (run once), the eight
slice cases of test_bicubic_adjoint_walk fail and its other 24 pass; of the earlier tests only four whole-network goldens of
tests/test_hip_parity.py notice, test_bicubic_adjoint_kernels_vs_torch does not.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import glue_cases as Gc
from pbml_mantle_convection_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7B
f32, f64 = torch.float32, torch.float64
NAN = float("nan")
MCDT = {"f32": L.MC_F32, "bf16": L.MC_BF16, "f16": L.MC_MIX16}
PRECS = ("f32", "bf16", "mix16")
MCPREC = {"f32": L.MC_F32, "bf16": L.MC_BF16, "mix16": L.MC_MIX16}
WORST = {}


def report(family, what, worst):
    WORST[family] = max(WORST.get(family, 0.0), float(worst))
    print(f"\n{family}: {what}: worst err / bound {float(worst):.3g}")


class Guarded:
    """A tensor between two sentinel bands inside one larger allocation (restated from tests/test_hip_loss_kernels.py)."""

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

    def untouched(self, what, index=Ellipsis):
        """The slice comes back bit-identical to what it held before the launch."""
        torch.cuda.synchronize()
        assert Gc.same_bits(self.t[index].contiguous(), self.before[index].contiguous()), f"{what} was written"


def cb8_dev(x, dt):
    """[N, C8 * 8, H, W] f64 -> CB8 device tensor of the storage type (NaN stays NaN)."""
    return Gc.to_cb8(x).to(Gc.DT[dt]).to(DEV).contiguous()


def nchw(t):
    """CB8 tensor (CPU) -> [N, C8 * 8, H, W] f64."""
    return Gc.from_cb8(t.double())


@functools.lru_cache(maxsize=None)
def dev_tables(n_in, n_out):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in Gc.tables(n_in, n_out)]


def grad_src(g, src, dt, **slice_kw):
    """(device buffer, GradSrc) for g [N, C8 * 8, h, w] held as `src` describes."""
    buf, tot, off = Gc.src_buffer(g, src, **slice_kw)
    d = buf.to(Gc.DT[dt]).to(DEV).contiguous()
    kind = {"plain": L.GSRC_PLAIN, "padfold": L.GSRC_PADFOLD, "plain_pool": L.GSRC_PLAIN_POOL, "padfold_pool": L.GSRC_PADFOLD_POOL}[src.kind]
    return d, L.GradSrc(L.ptr(d), kind, src.pad, L.PAD_MODES["reflect"], src.pool, g.shape[2], g.shape[3], tot, off)


# =============================================================================================================================
# converters
# =============================================================================================================================
@pytest.mark.parametrize("mode", Gc.PAD_MODES)
@pytest.mark.parametrize("H,W,pad_w", Gc.PACK_SHAPES)
@pytest.mark.parametrize("c,src_c", Gc.PACK_CHANNELS)
def test_pack_nchw(c, src_c, H, W, pad_w, mode):
    """src_c > c, the width frame in each pad mode, chan_scale: one f32 product and the store, bit for bit; zeros in the pad columns
    of the zeros mode and in the lanes past c."""
    x, cs = Gc.pack_inputs(c, src_c, H, W)
    xd, csd = x.float().to(DEV), cs.float().to(DEV)
    for dt in Gc.DT:
        for scale in (csd, None):
            out = Guarded((Gc.N, (c + 7) // 8, H, W + 2 * pad_w, 8), Gc.DT[dt])
            L.call("mc_pack_nchw", L.ptr(xd), Gc.N, c, src_c, H, W, pad_w, L.PAD_MODES[mode], L.ptr(scale), MCDT[dt], out.ptr, L.stream())
            got = nchw(out.cpu("mc_pack_nchw"))
            Gc.check_pack(x, cs if scale is not None else None, c, pad_w, mode, dt, got, f"mc_pack_nchw c {c}/{src_c} {H}x{W}+{pad_w} {mode} {dt}")
            assert not bool(got[:, c:].any())
            if mode == "zeros" and pad_w:
                assert not bool(got[..., :pad_w].any()) and not bool(got[..., W + pad_w:].any())
    report("converters", "mc_pack_nchw", 0.0)


@pytest.mark.parametrize("H,W,crop", Gc.UNPACK_SHAPES)
@pytest.mark.parametrize("c", Gc.UNPACK_CHANNELS)
def test_unpack_nchw(c, H, W, crop):
    """crop_w and mean_nc (the subtract_mean head): one f32 difference, bit for bit; the lanes past c never reach the output."""
    for dt in Gc.DT:
        x, mean = Gc.unpack_inputs(c, H, W, dt)
        xd, md = cb8_dev(x, dt), mean.float().to(DEV)
        for m in (md, None):
            out = Guarded((Gc.N, c, H, W - 2 * crop), f32)
            L.call("mc_unpack_nchw", L.ptr(xd), Gc.N, c, H, W, crop, L.ptr(m), MCDT[dt], out.ptr, L.stream())
            Gc.compare_exact(out.cpu("mc_unpack_nchw"), Gc.unpack_ref(x, mean if m is not None else None, c, crop),
                             f"mc_unpack_nchw c {c} {H}x{W} crop {crop} {dt}")
    report("converters", "mc_unpack_nchw", 0.0)


@pytest.mark.parametrize("H,W,crop", Gc.UNPACK_SHAPES)
@pytest.mark.parametrize("c", Gc.UNPACK_CHANNELS)
def test_pack_grad_nchw(c, H, W, crop):
    """g - mean, and 0 - mean in the cropped columns, bit for bit; with the mean from mc_sum_hw it is the f64 gradient of
    crop(y - mean_HW(y)) within the bound."""
    g, mean = Gc.pack_grad_inputs(c, H, W, crop)
    gd, md = g.float().to(DEV), mean.float().to(DEV)
    worst = 0.0
    for prec in PRECS:
        dt = Gc.GRAD_DT[prec]
        for m in (md, None):
            out = Guarded((Gc.N, (c + 7) // 8, H, W, 8), Gc.DT[dt])
            L.call("mc_pack_grad_nchw", L.ptr(gd), Gc.N, c, H, W, crop, L.ptr(m), MCPREC[prec], out.ptr, L.stream())
            Gc.check_pack_grad(g, mean if m is not None else None, c, crop, dt, nchw(out.cpu("mc_pack_grad_nchw")),
                               f"mc_pack_grad_nchw c {c} {H}x{W} crop {crop} {prec}")
        ms = Guarded((Gc.N * c,), f32)
        L.call("mc_sum_hw", L.ptr(gd), Gc.N * c, H * (W - 2 * crop), 1.0 / (H * W), ms.ptr, L.stream())
        ms.cpu("mc_sum_hw")
        out = Guarded((Gc.N, (c + 7) // 8, H, W, 8), Gc.DT[dt])
        L.call("mc_pack_grad_nchw", L.ptr(gd), Gc.N, c, H, W, crop, ms.ptr, MCPREC[prec], out.ptr, L.stream())
        worst = max(worst, Gc.check_pack_grad_mean(g, c, H, W, crop, dt, nchw(out.cpu("mc_pack_grad_nchw"))))
    report("converters", f"mc_sum_hw -> mc_pack_grad_nchw c {c} {H}x{W} crop {crop}", worst)


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("hw", Gc.SUM_HW)
def test_sum_hw(hw, offset):
    """The float4 path (hw % 4 == 0 from a 16-byte aligned base) and the scalar path (every other hw; the same hw from a base one
    float further on)."""
    x = Gc.randn((Gc.SUM_NC, hw), 7 + hw)
    hold = torch.zeros((Gc.SUM_NC * hw + 4,), dtype=f32, device=DEV)
    assert hold.data_ptr() % 16 == 0
    xd = hold[offset:offset + Gc.SUM_NC * hw]
    xd.copy_(x.reshape(-1).float())
    out = Guarded((Gc.SUM_NC,), f32)
    scale = 1.0 / 3.0
    L.call("mc_sum_hw", L.ptr(xd), Gc.SUM_NC, hw, scale, out.ptr, L.stream())
    w = Gc.check_sum_hw(x, float(np.float32(scale)), Gc.sum_takes_vec(hw, offset), out.cpu("mc_sum_hw"), f"mc_sum_hw hw {hw} offset {offset}")
    report("mc_sum_hw", f"hw {hw} offset {offset}", w)


# =============================================================================================================================
# mc_rect_copy, mc_gsrc_sum
# =============================================================================================================================
@pytest.mark.parametrize("dt", list(Gc.DT))
def test_rect_copy(dt):
    """Plain copy, accumulate (one f32 sum, then the store), a NULL source (zero fill; with accumulate the identity), offset and
    full-size rectangles: the whole destination bit for bit, so that nothing outside the rectangle moved."""
    src, dst = Gc.rect_inputs(dt)
    sd = cb8_dev(src, dt)
    (hs, ws), (hd, wd) = Gc.RECT_SRC, Gc.RECT_DST
    for r in Gc.RECTS:
        for with_src in (True, False):
            for acc in (0, 1):
                out = Guarded((Gc.N, 2, hd, wd, 8), Gc.DT[dt], fill=Gc.to_cb8(dst))
                L.call("mc_rect_copy", L.ptr(sd) if with_src else None, hs, ws, r["sy"], r["sx"], out.ptr, hd, wd, r["dy"], r["dx"], r["rh"], r["rw"],
                       Gc.N, Gc.C, acc, MCDT[dt], L.stream())
                what = f"mc_rect_copy {r} src {with_src} accumulate {acc} {dt}"
                Gc.check_rect(src if with_src else None, dst, r, acc, dt, nchw(out.cpu(what)), what)
                if not with_src and acc:
                    out.untouched(what)
                keep = torch.ones((hd, wd), dtype=torch.bool)
                keep[r["dy"]:r["dy"] + r["rh"], r["dx"]:r["dx"] + r["rw"]] = False
                assert Gc.same_bits(out.t[:, :, keep.to(DEV)], out.before[:, :, keep.to(DEV)]), what + ": written outside the rectangle"
    report("mc_rect_copy", dt, 0.0)


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("g1", Gc.GSUM_G1, ids=lambda s: "none" if s is None else f"{s.kind}{s.pool}")
@pytest.mark.parametrize("g0", Gc.GSUM_G0, ids=lambda s: s.kind + ("_slice" if s.sliced else ""))
def test_gsrc_sum(g0, g1, dt):
    """PLAIN, PADFOLD and a slice of a five-block tensor, plus nothing, or a pooled source with pool 2, pool 3 (the division path)
    or a padded pooled one: floor mode leaves the odd row and column of 9 x 13 without a pooled term."""
    H, W = Gc.GSUM_HW
    a, b = Gc.gsum_inputs(g1, dt)
    hold0, s0 = grad_src(a, g0, dt, **Gc.GSUM_SLICE)
    hold1, s1 = (None, None) if g1 is None else grad_src(b, g1, dt)
    out = Guarded((Gc.N, 2, H, W, 8), Gc.DT[dt])
    L.call("mc_gsrc_sum", C.byref(s0), C.byref(s1) if s1 is not None else None, Gc.N, Gc.C, H, W, MCDT[dt], out.ptr, L.stream())
    what = f"mc_gsrc_sum {g0} + {g1} {dt}"
    report("mc_gsrc_sum", what, Gc.check_gsum(a, b, g1, dt, nchw(out.cpu(what)), what))


# =============================================================================================================================
# the padding adjoint
# =============================================================================================================================
def run_fold(before, H, W, p, mode, dt, c=None):
    n, cp = before.shape[:2]
    buf = Guarded((n, cp // 8, H + 2 * p, W + 2 * p, 8), Gc.DT[dt], fill=Gc.to_cb8(before))
    L.call("mc_fold_padded", buf.ptr, n, c or cp, H, W, p, L.PAD_MODES[mode], MCDT[dt], L.stream())
    return buf


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("mode", Gc.FOLD_MODES)
@pytest.mark.parametrize("H,W,p", Gc.FOLD_CASES)
def test_fold_padded(H, W, p, mode, dt):
    """The `all` form, side = 0, the general form and two blocks in x, reflect and replicate (its nine-source corner), against
    autograd of F.pad; the halo and everything outside the frame bit for bit."""
    before = Gc.fold_inputs(H, W, p, dt)
    what = f"mc_fold_padded {H}x{W} pad {p} {mode} {dt}"
    buf = run_fold(before, H, W, p, mode, dt, c=Gc.C)
    report("mc_fold_padded", what, Gc.check_fold(before, nchw(buf.cpu(what)), p, mode, dt, what))
    halo = torch.ones((H + 2 * p, W + 2 * p), dtype=torch.bool)
    halo[p:p + H, p:p + W] = False
    assert Gc.same_bits(buf.t[:, :, halo.to(DEV)], buf.before[:, :, halo.to(DEV)]), what + ": the halo"
    inner = ~Gc.frame_mask(H, W, p)
    if bool(inner.any()):
        sel = torch.zeros_like(halo)
        sel[p:p + H, p:p + W] = inner
        assert Gc.same_bits(buf.t[:, :, sel.to(DEV)], buf.before[:, :, sel.to(DEV)]), what + ": outside the frame"


@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_fold_padded_nothing_to_fold(dt):
    """Zero padding and pad = 0 leave the buffer as it is."""
    H, W = 7, 8
    for p, mode in ((2, "zeros"), (0, "reflect"), (0, "zeros")):
        buf = run_fold(Gc.fold_inputs(H, W, p, dt), H, W, p, mode, dt)
        buf.cpu("mc_fold_padded")
        buf.untouched(f"mc_fold_padded pad {p} {mode}")


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("mode", Gc.FOLD_MODES)
@pytest.mark.parametrize("c0,c1", Gc.FOLD2_CHANNELS)
@pytest.mark.parametrize("H,W,p", [(3, 9, 2), (7, 8, 2), (40, 50, 2), (5, 6, 1)])
def test_fold_padded2(H, W, p, c0, c1, mode, dt):
    """Two buffers in one launch (the `cb >= C8a` switch): each against the reference, and bit-equal to two single calls."""
    worst = 0.0
    befores = [Gc.fold_inputs(H, W, p, dt, c=(c + 7) // 8 * 8, seed=s) for c, s in ((c0, 1), (c1, 2))]
    bufs = [Guarded((Gc.N, b.shape[1] // 8, H + 2 * p, W + 2 * p, 8), Gc.DT[dt], fill=Gc.to_cb8(b)) for b in befores]
    L.call("mc_fold_padded2", bufs[0].ptr, c0, bufs[1].ptr, c1, Gc.N, H, W, p, L.PAD_MODES[mode], MCDT[dt], L.stream())
    for k, (b, buf, c) in enumerate(zip(befores, bufs, (c0, c1))):
        what = f"mc_fold_padded2 buffer {k} ({c0}, {c1}) {H}x{W} pad {p} {mode} {dt}"
        worst = max(worst, Gc.check_fold(b, nchw(buf.cpu(what)), p, mode, dt, what))
        single = run_fold(b, H, W, p, mode, dt, c=c)
        single.cpu(what)
        assert Gc.same_bits(buf.t, single.t), what + ": differs from the single call"
    report("mc_fold_padded", f"two buffers ({c0}, {c1}) {H}x{W} pad {p} {mode} {dt}", worst)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mode", Gc.FOLD_MODES)
@pytest.mark.parametrize("H,W,p", Gc.FOLD_CASES)
def test_fold_padded_dz(H, W, p, mode, prec):
    """The frame turned into dz = fold x act'(y sc + sh) in place, gelu and relu, coef given and NULL, f16 y with a bf16 buffer in
    the mixed mode; the per-block (sum dz, sum dz yhat) partials at slots [2, 2 + blocks) of blocks + 5, the other slots untouched."""
    blocks = Gc.fold_blocks(H, W, p)
    stride = blocks + Gc.DZ_EXTRA
    gdt, ydt = Gc.GRAD_DT[prec], Gc.FWD_DT[prec]
    w1 = w2 = 0.0
    for act in Gc.DZ_ACTS:
        for with_coef in (True, False):
            before, y, coef = Gc.dz_inputs(H, W, p, prec, with_coef)
            buf = Guarded((Gc.N, 2, H + 2 * p, W + 2 * p, 8), Gc.DT[gdt], fill=Gc.to_cb8(before))
            yd = cb8_dev(y, ydt)
            cd = coef.float().to(DEV).contiguous() if with_coef else None
            part = Guarded((Gc.N, stride, 16, 2), f32, fill=Gc.DZ_PREFILL)
            L.call("mc_fold_padded_dz", buf.ptr, Gc.N, Gc.C, H, W, p, L.PAD_MODES[mode], MCPREC[prec], L.ptr(yd), L.ptr(cd), L.ACTS[act],
                   part.ptr, stride, Gc.DZ_FIRST, L.stream())
            what = f"mc_fold_padded_dz {H}x{W} pad {p} {mode} {act} coef {with_coef} {prec}"
            pt = part.cpu(what).double()
            part.untouched(what + ": slots before the launch's", (slice(None), slice(0, Gc.DZ_FIRST)))
            part.untouched(what + ": slots behind the launch's", (slice(None), slice(Gc.DZ_FIRST + blocks, stride)))
            sums = pt[:, Gc.DZ_FIRST:Gc.DZ_FIRST + blocks].sum(1)
            a, b = Gc.check_fold_dz(before, nchw(buf.cpu(what)), sums, y, coef, p, mode, act, prec, what)
            w1, w2 = max(w1, a), max(w2, b)
    report("mc_fold_padded_dz dz", f"{H}x{W} pad {p} {mode} {prec}", w1)
    report("mc_fold_padded_dz partials", f"{H}x{W} pad {p} {mode} {prec}", w2)


# =============================================================================================================================
# bicubic forward
# =============================================================================================================================
def run_fwd(b, x, coef=None, act="none"):
    ty, tx = dev_tables(b.hi, b.ho), dev_tables(b.wi, b.wo)
    xd = cb8_dev(x, b.dt)
    out = Guarded((b.n, x.shape[1] // 8, b.ho, b.wo, 8), Gc.DT[b.dt])
    if coef is None and act == "none":
        L.call("mc_bicubic_fwd", L.ptr(xd), b.n, b.c, b.hi, b.wi, b.ho, b.wo, L.ptr(ty[0]), L.ptr(ty[1]), L.ptr(tx[0]), L.ptr(tx[1]), MCDT[b.dt],
               out.ptr, L.stream())
    else:
        cd = coef.float().to(DEV).contiguous() if coef is not None else None
        L.call("mc_bicubic_fwd_act", L.ptr(xd), L.ptr(cd), L.ACTS[act], b.n, b.c, b.hi, b.wi, b.ho, b.wo, L.ptr(ty[0]), L.ptr(ty[1]), L.ptr(tx[0]),
               L.ptr(tx[1]), MCDT[b.dt], out.ptr, L.stream())
    return nchw(out.cpu("bicubic forward " + b.tag))


@pytest.mark.parametrize("b", Gc.FWD_DOWN, ids=lambda b: b.tag)
def test_bicubic_forward_downsampling(b):
    """ho < hi or wo < wi: the tiled kernel k_bicubic_fwd and, where a tile's taps leave its 12 x 36 window, bicubic_direct."""
    got = run_fwd(b, Gc.fwd_input(b))
    report("bicubic forward, tiled", b.tag, Gc.check_fwd(b, got))
    assert not bool(got[:, b.c:].any())


@pytest.mark.parametrize("b", Gc.FWD_OLD + [Gc.FWD_LONG], ids=lambda b: b.tag)
def test_bicubic_forward_walk(b):
    """The shapes of test_bicubic_forward_kernel_vs_torch under the derived bound, and the long walk: 4 chunks of 32 output rows."""
    got = run_fwd(b, Gc.fwd_input(b))
    report("bicubic forward, walk", b.tag, Gc.check_fwd(b, got))


@pytest.mark.parametrize("with_coef", (True, False))
@pytest.mark.parametrize("b", Gc.FWD_ACT, ids=lambda b: b.tag)
def test_bicubic_forward_act(b, with_coef):
    """The producer's affine and GELU applied while the window is staged, in the storage type."""
    x, coef = Gc.fwd_act_inputs(b, with_coef)
    got = run_fwd(b, x, coef, "gelu")
    report("bicubic forward with activation", b.tag + f" coef {with_coef}", Gc.check_fwd_act(b, "gelu", with_coef, got))


# =============================================================================================================================
# bicubic adjoint
# =============================================================================================================================
def run_adjoint(b, kernel, src, plain_entry=False):
    g = Gc.adj_input(b)
    hold, gs = grad_src(g, src, b.dt)
    ty, tx = dev_tables(b.hi, b.ho), dev_tables(b.wi, b.wo)
    c8 = g.shape[1] // 8
    out = Guarded((b.n, c8, b.hi, b.wi, 8), Gc.DT[b.dt])
    mcdt = L.MC_MIX16 if (b.dt == "bf16" and src.sliced) else MCDT[b.dt]            # the mixed mode's gradients are bf16 too
    mty, mtx = Gc.max_taps(b.hi, b.ho), Gc.max_taps(b.wi, b.wo)
    what = f"bicubic adjoint ({kernel}) {b.tag} from {src}"
    if kernel == "walk":
        L.call("mc_bicubic_bwd_walk", C.byref(gs), b.n, b.c, b.hi, b.wi, b.ho, b.wo, L.ptr(ty[0]), L.ptr(ty[1]), L.ptr(ty[2]), L.ptr(ty[3]),
               L.ptr(tx[2]), L.ptr(tx[3]), L.ptr(tx[4]), mtx, mcdt, out.ptr, L.stream())
    elif kernel == "taps" and plain_entry:
        L.call("mc_bicubic_bwd", C.byref(gs), b.n, b.c, b.hi, b.wi, b.ho, b.wo, L.ptr(ty[2]), L.ptr(ty[3]), L.ptr(ty[4]), L.ptr(tx[2]),
               L.ptr(tx[3]), L.ptr(tx[4]), mcdt, out.ptr, L.stream())
    elif kernel == "taps":
        L.call("mc_bicubic_bwd_taps", C.byref(gs), b.n, b.c, b.hi, b.wi, b.ho, b.wo, L.ptr(ty[2]), L.ptr(ty[3]), L.ptr(ty[4]), L.ptr(tx[2]),
               L.ptr(tx[3]), L.ptr(tx[4]), mty, mtx, mcdt, out.ptr, L.stream())
    else:
        ws = Guarded((b.n, c8, b.hi, b.wo, 8), f32)
        L.call("mc_bicubic_bwd_separable", C.byref(gs), b.n, b.c, b.hi, b.wi, b.ho, b.wo, L.ptr(ty[2]), L.ptr(ty[3]), L.ptr(ty[4]), L.ptr(tx[2]),
               L.ptr(tx[3]), L.ptr(tx[4]), mcdt, ws.ptr, out.ptr, L.stream())
        assert bool(torch.isfinite(ws.cpu(what + ": workspace")).all()), what + ": the workspace was not filled"
    return Gc.check_adjoint(b, kernel, nchw(out.cpu(what)), what)


SRC_IDS = [f"{s.kind}{s.pad}" + ("_slice" if s.sliced else "") for s in Gc.ADJ_SOURCES]


@pytest.mark.parametrize("src", Gc.ADJ_SOURCES, ids=SRC_IDS)
@pytest.mark.parametrize("b", Gc.WALK_CASES + [Gc.AGREE_CASE, Gc.WALK_LONG], ids=lambda b: b.tag)
def test_bicubic_adjoint_walk(b, src):
    """Column strips of the SW = 128 and SW = 256 instantiations, the BXT = 12 one, and the long walk (16 input rows per chunk)."""
    report("bicubic adjoint, walk", f"{b.tag} from {src}", run_adjoint(b, "walk", src))


@pytest.mark.parametrize("src", Gc.ADJ_SOURCES, ids=SRC_IDS)
@pytest.mark.parametrize("b", Gc.TAPS_CASES + [Gc.TAPS_GATHER, Gc.TAPS_PERSISTENT], ids=lambda b: b.tag)
def test_bicubic_adjoint_taps(b, src):
    """The four instantiations of k_bicubic_bwd, the gather fallback (16-entry lists) and the persistent loop (30 tiles, 24 blocks)."""
    report("bicubic adjoint, taps", f"{b.tag} from {src}", run_adjoint(b, "taps", src))


@pytest.mark.parametrize("src", Gc.ADJ_SOURCES, ids=SRC_IDS)
def test_bicubic_adjoint_plain_entry(src):
    """mc_bicubic_bwd: max_taps (0, 0), the (12, 12) instantiation."""
    b = Gc.TAPS_PLAIN
    report("bicubic adjoint, taps", f"mc_bicubic_bwd {b.tag} from {src}", run_adjoint(b, "taps", src, plain_entry=True))


@pytest.mark.parametrize("src", Gc.ADJ_SOURCES, ids=SRC_IDS)
@pytest.mark.parametrize("b", Gc.SEP_CASES + [Gc.AGREE_CASE], ids=lambda b: b.tag)
def test_bicubic_adjoint_separable(b, src):
    """The production route of NewFluidNet's x4 / x8 / x16 levels, its f32 workspace between sentinel bands."""
    report("bicubic adjoint, separable", f"{b.tag} from {src}", run_adjoint(b, "separable", src))


def test_worst_per_family():
    """Prints the table of this file's docstring (after the tests above, in file order)."""
    print("\nworst err / bound per family:")
    for k, v in WORST.items():
        print(f"  {k:36s} {v:.3g}")

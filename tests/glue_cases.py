"""Case tables, f64 references, derived bounds, comparison functions and mutants for the layout, fold, copy and bicubic kernels of
csrc/layout.hip, csrc/bicubic.hip and csrc/groupnorm.hip (tests/test_hip_glue_kernels.py on the GPU, tests/test_glue_cases_host.py on the CPU).  Nothing here touches a
device: the GPU file hands what a kernel wrote to the `check_*` functions below, the host file hands them the mutants.

Inputs are drawn with a seeded generator and rounded to the storage type first (f32, bf16, f16), so a reference sees what the
kernel reads.  In the mixed mode the forward tensors are f16 and the gradient tensors bf16.

Bounds.  U = 2^-24.  The library is built with -ffp-contract=off: every operation rounds once.  A bound is
gamma(K) x (the reference's expression on absolute values), gamma(K) = K U / (1 - K U), K the number of roundings on the kernel's
longest chain, and the store adds u (|ref| + E): u = 2^-8 bf16, 2^-11 f16, 0 f32 (tests/conv_variants.py UNIT; an f16 store adds
2^-25, half the subnormal spacing, because inputs drawn around zero produce results below 2^-14).  The counts, from the source:

  exact        k_pack_nchw: x * chan_scale, one f32 product, then the store.  k_unpack_nchw: v - mean, one f32 difference into f32.
               k_pack_grad_nchw: g - mean (0 - mean in the cropped columns), then the store.  k_rect_copy: a move; `accumulate`
               is one f32 sum, then the store.  All asserted bit for bit against the same f32 operation in torch.
  K_SUM        k_sum_hw, 1024 threads: a thread adds its ceil(hw / 1024) values (the first addition, to 0, is exact), or on the
               float4 path four sums of ceil(hw / 4096) values and two levels to combine them; wave_sum is 6 levels, thread 0
               adds 16 wave totals (15 roundings) and multiplies by `scale` (1):  chain + 6 + 15 + 1.
  fold         k_fold_padded: the f32 sum of the cnt sources of a pixel in a fixed order, from 0: cnt - 1 roundings per pixel
               (cnt <= 9: the replicate corner at pad 2, 3 x 3 sources); a pixel with cnt = 1 is not written at all.
  fold_dz      k_fold_padded_dz: the same sum (E_acc), z = y sc + sh (2 roundings of |y sc| + |sh|), g = act'(z) within
               gn_cases.act_grad_error of the f64 derivative at the kernel's z, dz = acc g (1): E = E_acc |g| + |acc| E_g + U |dz|.
               Partials: s2 = dz (y - me) rs is 3 roundings more; wave_sum16 is 6 levels and the four waves add 3: K_PART = 9 on
               the sum of the |terms|, plus the per-pixel bounds of the terms.  A kink pixel (relu: |z| < 2^-20 (|y sc| + |sh|)) is
               left out of the dz comparison and adds |acc| (and |acc yhat|) to the partials' bounds.
  K_GSUM       k_gsrc_sum: 0 + 1 g0 exact; + scale g1: the product is exact for pool 1 and 2 (scale 1, 1/4) and rounds for pool 3,
               where f32(1/9) is off by a rounding itself (2); the sum rounds (1):  1, or 3 with pool = 3.
  K_FWD = 17   bicubic forward, walk and tiled kernel: 4 products and 3 sums along x, the same along y (14), and the three sums
               that merge the weights of clamped rows (3); bicubic_direct: w = wy wx (1), 16 products w v on one chain of 15
               sums: 17 as well.  mc_bicubic_fwd_act: the staged value is act(x sc + sh) (gn_cases' bound E_a) rounded to the
               storage type; against the rounded reference that is E_a + u (2 |a| + E_a), carried through the absolute-value
               operator, before the 17.
  adjoint      ny, nx: the longest transposed tap lists of the case (entries in y, entries in x).
               walk:      ny products and sums into the register window, 3 sums where a clamped row merges weights, nx products
                          and sums of the x pass:  2 (ny + nx) + 3.  Its y operator is the FORWARD table (what the kernel reads),
                          merged in f64; the absolute-value twin merges |w|.
               taps:      the two passes, 2 (ny + nx); a pixel whose lists leave the 40 x 40 window or the BYT / BXT slots gathers
                          ny nx terms w = wy wx (1), w v (1) on one chain of sums: ny nx + 1.  The larger of the two per case.
               separable: the y pass into f32 (stored exactly), the x pass:  2 (ny + nx).
"""
import functools
import os
import sys
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gn_cases as G  # noqa: E402
from conv_variants import UNIT  # noqa: E402
from pbml_mantle_convection_amd.engine import bicubic_tables  # noqa: E402

f64 = torch.float64
U = 2.0 ** -24
NAN = float("nan")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
GRAD_DT = {"f32": "f32", "bf16": "bf16", "mix16": "bf16"}             # precision of a layer -> its gradient tensors
FWD_DT = {"f32": "f32", "bf16": "bf16", "mix16": "f16"}               # ... -> its forward tensors
F16_HALF_SPACING = 2.0 ** -25
MAX_SHARE = 0.05                                                       # of a case a kink rule may leave out (loss_cases.MAX_SHARE)
K_FWD, K_PART = 17, 9
N = 2
C = 12                                                                 # one full and one ragged channel block
PAD_F = {"zeros": "constant", "reflect": "reflect", "replicate": "replicate"}


def cdiv(a, b):
    return -(-a // b)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- inputs, layout ---------------------------------------------------------------------------------------------------------
def rq(x, dt):
    """x rounded to the storage type dt (round to nearest even), as f64."""
    return x.to(DT[dt]).double()


def randn(shape, seed, dt="f32", scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(int(seed))
    return rq(torch.randn(shape, generator=g, dtype=f64) * scale + shift, dt)


def to_cb8(x, lanes=0.0):
    """[N, C, H, W] -> CB8 [N][ceil(C / 8)][H][W][8]; lanes past C hold `lanes`."""
    n, c, h, w = x.shape
    c8 = (c + 7) // 8
    full = torch.full((n, c8 * 8, h, w), lanes, dtype=x.dtype)
    full[:, :c] = x
    return full.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def from_cb8(t):
    """CB8 [N][C8][H][W][8] -> [N, C8 * 8, H, W]."""
    n, c8, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)


def store_bound(E, ref, dt):
    """The bound E on the f32 value, after the store to dt."""
    E = torch.as_tensor(E, dtype=f64)
    return E + UNIT[DT[dt]] * (ref.abs() + E) + (F16_HALF_SPACING if dt == "f16" else 0.0)


# ---- comparisons ------------------------------------------------------------------------------------------------------------
def compare(got, ref, tol, what):
    """Every element finite and within tol of ref.  Returns the worst err / tol (0 / 0 counts as 0: an exact element)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements are not finite"
    tol = torch.as_tensor(tol, dtype=f64).expand_as(ref)
    err = (got - ref).abs()
    bad = err > tol
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(bad.any()):
        i = int(torch.argmax(ratio.reshape(-1)))
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst err / bound {worst:.3g} at "
                             f"{idx}: got {float(got[idx]):.9g}, reference {float(ref[idx]):.9g}, bound {float(tol[idx]):.3g}")
    return worst


def compare_exact(got, ref, what):
    """Bit for bit (as values: a NaN fails, -0 equals 0)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements are not finite"
    bad = got != ref
    if bool(bad.any()):
        idx = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {float(got[idx]):.9g}, "
                             f"expected {float(ref[idx]):.9g}")
    return 0.0


def same_bits(a, b):
    """Two tensors of one dtype hold the same bytes (NaN payloads included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# =============================================================================================================================
# NCHW converters, mc_sum_hw
# =============================================================================================================================
PACK_CHANNELS = [(3, 5), (8, 8), (12, 12)]                             # (c, src_c)
PACK_SHAPES = [(5, 4, 3), (6, 7, 0), (6, 7, 3)]                        # (H, W, pad_w)
PAD_MODES = ("zeros", "replicate", "reflect")
UNPACK_CHANNELS = (3, 12)
UNPACK_SHAPES = [(5, 9, 3), (6, 7, 0)]                                 # (H, W, crop)
SUM_HW = (1, 35, 64, 4100)
SUM_NC = 6


def pack_inputs(c, src_c, H, W):
    return randn((N, src_c, H, W), 11 + c + 10 * H), randn((c,), 12 + c, scale=0.5, shift=1.5)


def pack_ref(x, cs, c, pad_w, mode, dt):
    """[N, C8 * 8, H, W + 2 pad_w] of mc_pack_nchw: one f32 product, the store, the pad columns, zero lanes."""
    v = x[:, :c].float()
    if cs is not None:
        v = v * cs.float().view(1, -1, 1, 1)
    v = v.to(DT[dt]).double()
    if pad_w:
        v = F.pad(v, (pad_w, pad_w, 0, 0), mode=PAD_F[mode])
    return from_cb8(to_cb8(v))


def check_pack(x, cs, c, pad_w, mode, dt, got, what):
    return compare_exact(got, pack_ref(x, cs, c, pad_w, mode, dt), what)


def unpack_inputs(c, H, W, dt):
    """The CB8 tensor as [N, C8 * 8, H, W] (lanes past c hold data of their own: they must not reach the output) and a mean."""
    c8 = (c + 7) // 8
    return randn((N, c8 * 8, H, W), 21 + c + 10 * H, dt), randn((N, c), 22 + c, scale=0.3)


def unpack_ref(x, mean, c, crop):
    v = x[:, :c].float()
    if mean is not None:
        v = v - mean.float().view(N, c, 1, 1)
    return v[:, :, :, crop:x.shape[3] - crop].double()


def pack_grad_inputs(c, H, W, crop):
    return randn((N, c, H, W - 2 * crop), 31 + c + 10 * H), randn((N, c), 32 + c, scale=0.3)


def pack_grad_ref(g, mean, c, crop, dt, mutant=None):
    """[N, C8 * 8, H, W]: g - mean inside, 0 - mean in the cropped columns, zero lanes past c."""
    v = F.pad(g.float(), (crop, crop, 0, 0))
    if mean is not None:
        m = mean.float().view(N, c, 1, 1)
        v = v - m
        if mutant == "crop_zero" and crop:
            v[..., :crop] = 0.0
            v[..., v.shape[3] - crop:] = 0.0
    return from_cb8(to_cb8(v.to(DT[dt]).double()))


def check_pack_grad(g, mean, c, crop, dt, got, what):
    return compare_exact(got, pack_grad_ref(g, mean, c, crop, dt), what)


def sum_chain(hw, vec):
    return (cdiv(hw // 4, 1024) - 1 + 2) if vec else (cdiv(hw, 1024) - 1)


def k_sum(hw, vec):
    return max(0, sum_chain(hw, vec)) + 6 + 15 + 1


def sum_takes_vec(hw, offset_floats):
    return hw % 4 == 0 and offset_floats % 4 == 0


def check_sum_hw(x, scale, vec, got, what):
    """x [nc, hw] f64 of f32 values; got [nc]."""
    ref = x.sum(1) * scale
    return compare(got, ref, gamma(k_sum(x.shape[1], vec)) * x.abs().sum(1) * abs(scale), what)


def mean_grad_ref(g, H, W, crop):
    """(gradient, its absolute-value twin) of sum <g, crop(y - mean_HW(y))> with respect to y [N, c, H, W], in f64."""
    gp = F.pad(g, (crop, crop, 0, 0))
    m, ma = gp.sum((2, 3), keepdim=True) / (H * W), gp.abs().sum((2, 3), keepdim=True) / (H * W)
    return gp - m, gp.abs() + ma


def check_pack_grad_mean(g, c, H, W, crop, dt, got):
    """mc_sum_hw(g, scale = 1 / (H W)) -> mc_pack_grad_nchw against the f64 gradient: K_SUM for the mean, its product with the
    scale is counted there, one rounding for the difference."""
    ref, mag = mean_grad_ref(g, H, W, crop)
    hw = H * (W - 2 * crop)
    k = max(k_sum(hw, True), k_sum(hw, False)) + 1
    full, fmag = from_cb8(to_cb8(ref)), from_cb8(to_cb8(mag))
    return compare(got, full, store_bound(gamma(k) * fmag, full, dt), f"pack_grad with the mean of mc_sum_hw, c {c} {H}x{W} crop {crop} {dt}")


# =============================================================================================================================
# mc_rect_copy
# =============================================================================================================================
RECT_SRC, RECT_DST = (9, 11), (12, 13)
RECTS = [dict(sy=2, sx=3, dy=1, dx=4, rh=5, rw=6), dict(sy=0, sx=0, dy=0, dx=0, rh=9, rw=11), dict(sy=0, sx=0, dy=3, dx=2, rh=9, rw=11)]


def rect_inputs(dt):
    c8 = (C + 7) // 8
    return randn((N, c8 * 8, *RECT_SRC), 41, dt), randn((N, c8 * 8, *RECT_DST), 42, dt)


def rect_ref(src, dst, r, accumulate, dt, mutant=None):
    """The whole destination after mc_rect_copy(src or None, ..., accumulate)."""
    out = dst.clone()
    ys, xs = slice(r["dy"], r["dy"] + r["rh"]), slice(r["dx"], r["dx"] + r["rw"])
    v = torch.zeros_like(out[:, :, ys, xs]) if src is None else src[:, :, r["sy"]:r["sy"] + r["rh"], r["sx"]:r["sx"] + r["rw"]]
    if accumulate and mutant != "no_accumulate":
        v = (v.float() + out[:, :, ys, xs].float()).to(DT[dt]).double()
    out[:, :, ys, xs] = v
    return out


def check_rect(src, dst, r, accumulate, dt, got, what):
    return compare_exact(got, rect_ref(src, dst, r, accumulate, dt), what)


# =============================================================================================================================
# gradient sources: PLAIN, PADFOLD, slices, pooled
# =============================================================================================================================
class Src(NamedTuple):
    kind: str            # plain | padfold | plain_pool | padfold_pool
    pad: int = 0
    pool: int = 1
    sliced: bool = False


def src_buffer(g, src, extra=2, off=1):
    """The CB8 tensor [N][c8_total][h + 2 pad][w + 2 pad][8] that holds g [N, C8 * 8, h, w] as `src` describes it: NaN in the halo and
    in the blocks of a wider tensor that are not this slice.  Returns (buffer, c8_total, cb_off)."""
    n, c, h, w = g.shape
    c8, p = c // 8, src.pad
    tot, o = (c8 + extra, off) if src.sliced else (c8, 0)
    buf = torch.full((n, tot, h + 2 * p, w + 2 * p, 8), NAN, dtype=f64)
    buf[:, o:o + c8, p:p + h, p:p + w] = to_cb8(g)
    return buf, (tot if src.sliced else 0), o


GSUM_HW = (9, 13)
GSUM_G0 = [Src("plain"), Src("padfold", 2), Src("plain", sliced=True)]            # the slice: c8_total = 5, cb_off = 2
GSUM_G1 = [None, Src("plain_pool", 0, 2), Src("plain_pool", 0, 3), Src("padfold_pool", 2, 2)]
GSUM_SLICE = dict(extra=3, off=2)


def gsum_inputs(g1, dt):
    H, W = GSUM_HW
    a = randn((N, 16, H, W), 51, dt)
    b = None if g1 is None else randn((N, 16, H // g1.pool, W // g1.pool), 52 + g1.pool, dt)
    return a, b


def unpool(b, pool, H, W, mutant=None):
    """The adjoint of AvgPool(pool) in floor mode without its 1 / pool^2: the trailing rows and columns get nothing."""
    up = torch.zeros((b.shape[0], b.shape[1], H, W), dtype=f64)
    hh, ww = b.shape[2] * pool, b.shape[3] * pool
    up[:, :, :hh, :ww] = b.repeat_interleave(pool, 2).repeat_interleave(pool, 3)
    if mutant == "trailing_row":                      # the index clamped, not skipped (the row; at 9 / 3 there is only a column)
        if hh < H:
            up[:, :, hh:, :ww] = up[:, :, hh - 1:hh, :ww]
        else:
            up[:, :, :, ww:] = up[:, :, :, ww - 1:ww]
    return up


def gsum_ref(a, b, g1, mutant=None):
    if b is None:
        return a.clone(), a.abs(), 1
    up = unpool(b, g1.pool, a.shape[2], a.shape[3], mutant) / (g1.pool * g1.pool)
    return a + up, a.abs() + up.abs(), (3 if g1.pool == 3 else 1)


def check_gsum(a, b, g1, dt, got, what):
    ref, mag, k = gsum_ref(a, b, g1)
    return compare(got, ref, store_bound(gamma(k) * mag, ref, dt), what)


# =============================================================================================================================
# the padding adjoint: mc_fold_padded, mc_fold_padded2, mc_fold_padded_dz
# =============================================================================================================================
FOLD_CASES = [(3, 9, 2), (9, 3, 1), (6, 7, 2), (5, 6, 1), (7, 8, 2), (40, 50, 2)]          # (H, W, p)
FOLD_MODES = ("reflect", "replicate")
FOLD2_CHANNELS = [(8, 12), (20, 8)]


def fold_shape(H, W, p):
    """(all, total, side) of mc_fold_padded2 / fold_shape, restated."""
    t = p + 1
    al = int(H < 2 * t or W < 2 * t)
    side = 0 if al else (H - 2 * t) * 2 * t
    total = H * W if al else 2 * t * W + side
    return al, total, side


def fold_blocks(H, W, p):
    return cdiv(fold_shape(H, W, p)[1], 256)


def frame_mask(H, W, p):
    """The pixels mc_fold_padded_dz turns into dz: within p + 1 of the border."""
    t = p + 1
    m = torch.ones((H, W), dtype=torch.bool)
    if not fold_shape(H, W, p)[0]:
        m[t:H - t, t:W - t] = False
    return m


def fold_autograd(gp, p, mode):
    """The adjoint of F.pad(x, (p, p, p, p), mode) applied to the padded-domain gradient gp [N, C, H + 2 p, W + 2 p], by autograd."""
    n, c, Hp, Wp = gp.shape
    x = torch.zeros((n, c, Hp - 2 * p, Wp - 2 * p), dtype=f64, requires_grad=True)
    F.pad(x, (p, p, p, p), mode=PAD_F[mode]).backward(gp)
    return x.grad


def pad_source(n, p, mode, mutant=None):
    """Interior index that padded coordinate i - p reads, i = 0 .. n + 2 p - 1."""
    i = np.arange(-p, n + p)
    if mode == "replicate":
        j = np.clip(i, 0, n - 1)
    elif mutant == "edge_mirror":                     # mirrored about the edge, not about the last pixel
        j = np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    else:
        j = np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))
    return torch.from_numpy(np.clip(j, 0, n - 1).astype(np.int64))


def fold_index(gp, p, mode, mutant=None):
    """The same adjoint from the index maps (the form the mutants change)."""
    n, c, Hp, Wp = gp.shape
    H, W = Hp - 2 * p, Wp - 2 * p
    gp = gp.clone()
    if mutant == "no_diagonal":                       # the corner sums its row and its column of the halo only
        for ys in (slice(0, p), slice(Hp - p, Hp)):
            for xs in (slice(0, p), slice(Wp - p, Wp)):
                gp[:, :, ys, xs] = 0.0
    tmp = torch.zeros((n, c, H, Wp), dtype=f64).index_add_(2, pad_source(H, p, mode, mutant), gp)
    out = torch.zeros((n, c, H, W), dtype=f64).index_add_(3, pad_source(W, p, mode, mutant), tmp)
    if mutant == "skip_last_row":
        out[:, :, H - 1] = gp[:, :, p + H - 1, p:p + W]
    return out


def fold_inputs(H, W, p, dt, c=16, seed=0):
    return randn((N, c, H + 2 * p, W + 2 * p), 61 + H + 100 * W + seed, dt)


def fold_expected(before, p, mode, dt):
    """(reference, bound, mask of the pixels the kernel writes) on the interior."""
    ref = fold_autograd(before, p, mode)
    mag = fold_autograd(before.abs(), p, mode)
    cnt = fold_autograd(torch.ones_like(before), p, mode).round()
    return ref, store_bound(gamma(1) * (cnt - 1) * mag, ref, dt) * (cnt > 1), cnt > 1


def check_fold(before, after, p, mode, dt, what):
    """before / after: the whole padded buffer [N, C8 * 8, H + 2 p, W + 2 p] around mc_fold_padded.  The halo and every pixel with a
    single source come back as they were, bit for bit (values: both are finite inputs); the rest is within the bound."""
    Hp, Wp = before.shape[2:]
    H, W = Hp - 2 * p, Wp - 2 * p
    assert bool(torch.isfinite(after).all()), f"{what}: not finite"
    halo = torch.ones((Hp, Wp), dtype=torch.bool)
    halo[p:p + H, p:p + W] = False
    assert torch.equal(after[:, :, halo], before[:, :, halo]), f"{what}: the halo was written"
    ref, tol, written = fold_expected(before, p, mode, dt)
    inner_b, inner_a = before[:, :, p:p + H, p:p + W], after[:, :, p:p + H, p:p + W]
    assert torch.equal(inner_a[~written], inner_b[~written]), f"{what}: a pixel without halo sources was changed"
    outside = ~frame_mask(H, W, p)
    assert torch.equal(inner_a[:, :, outside], inner_b[:, :, outside]), f"{what}: a pixel outside the frame was changed"
    assert not bool(written[:, :, outside].any())
    return compare(inner_a, torch.where(written, ref, inner_b), tol, what)


def fold_mutant_after(before, p, mode, dt, mutant):
    """The padded buffer a kernel with `mutant` would leave."""
    H, W = before.shape[2] - 2 * p, before.shape[3] - 2 * p
    cnt = fold_autograd(torch.ones_like(before), p, mode).round()
    after = before.clone()
    inner = after[:, :, p:p + H, p:p + W]
    inner[:] = torch.where(cnt > 1, rq(fold_index(before, p, mode, mutant), dt), inner)
    return after


# ---- mc_fold_padded_dz ------------------------------------------------------------------------------------------------------
DZ_ACTS = ("gelu", "relu")
DZ_FIRST, DZ_EXTRA = 2, 5                            # part_first_block, part_stride_blocks - blocks
DZ_PREFILL = 0.25


def dz_inputs(H, W, p, prec, with_coef):
    """buf (padded, gradient type), y (forward type), coef4 [N][16][4] f32 or None."""
    gdt, ydt = GRAD_DT[prec], FWD_DT[prec]
    buf = fold_inputs(H, W, p, gdt, seed=7)
    y = randn((N, 16, H, W), 71 + H + 100 * W, ydt, scale=1.2, shift=0.2)
    coef = None
    if with_coef:
        g = torch.Generator().manual_seed(72 + H)
        sc = 0.8 + 0.4 * torch.rand((N, 16), generator=g, dtype=f64)
        sh = 0.3 * torch.randn((N, 16), generator=g, dtype=f64)
        me = 0.2 + 0.1 * torch.randn((N, 16), generator=g, dtype=f64)
        rs = 0.8 + 0.2 * torch.rand((N, 16), generator=g, dtype=f64)
        coef = rq(torch.stack([sc, sh, me, rs], -1), "f32")
    return buf, y, coef


class DzRef(NamedTuple):
    dz: torch.Tensor          # [N, 16, H, W] on the frame (elsewhere: the buffer's own interior)
    tol: torch.Tensor
    frame: torch.Tensor       # [H, W] bool
    kink: torch.Tensor        # [N, 16, H, W] bool: left out of the dz comparison
    sums: torch.Tensor        # [N, 16, 2]
    sums_tol: torch.Tensor


def dz_ref(buf, y, coef, p, mode, act, prec):
    n, c, Hp, Wp = buf.shape
    H, W = Hp - 2 * p, Wp - 2 * p
    one = torch.ones((n, c, 1, 1), dtype=f64)
    sc, sh, me, rs = [coef[:, :, i].view(n, c, 1, 1) for i in range(4)] if coef is not None else [one, 0 * one, 0 * one, 0 * one]
    acc, mag = fold_autograd(buf, p, mode), fold_autograd(buf.abs(), p, mode)
    cnt = fold_autograd(torch.ones_like(buf), p, mode).round()
    E_acc = gamma(1) * (cnt - 1) * mag
    z, A = y * sc + sh, (y * sc).abs() + sh.abs()
    Ez = 2 * U * A if coef is not None else 0 * A                       # y * 1 + 0 is exact
    gz = G.act_grad64(z, act)
    E_g = G.LIP2[act] * Ez + G.act_grad_error(z, act, "f32" if prec == "f32" else "bf16")
    dz = acc * gz
    E = E_acc * gz.abs() + (acc.abs() + E_acc) * E_g + U * dz.abs()
    frame = frame_mask(H, W, p)
    kink = (z.abs() < G.KINK_REL * A) & frame if act in G.JUMP else torch.zeros_like(z, dtype=torch.bool)
    yhat = (y - me) * rs
    t1, t2 = dz * frame, dz * yhat * frame
    E1 = torch.where(kink, acc.abs() * G.JUMP.get(act, 0.0), E) * frame
    E2 = E1 * yhat.abs() + 3 * U * t2.abs()
    sums = torch.stack([t1.sum((2, 3)), t2.sum((2, 3))], -1)
    stol = torch.stack([E1.sum((2, 3)) + gamma(K_PART) * t1.abs().sum((2, 3)), E2.sum((2, 3)) + gamma(K_PART) * t2.abs().sum((2, 3))], -1)
    inner = buf[:, :, p:p + H, p:p + W]
    return DzRef(torch.where(frame, dz, inner), store_bound(E, dz, GRAD_DT[prec]) * frame, frame, kink, sums, stol)


def check_fold_dz(before, after, sums, y, coef, p, mode, act, prec, what):
    """The padded buffer around mc_fold_padded_dz and the partials summed over the launch's slots [N, 16, 2]."""
    Hp, Wp = before.shape[2:]
    H, W = Hp - 2 * p, Wp - 2 * p
    r = dz_ref(before, y, coef, p, mode, act, prec)
    assert float(r.kink.sum()) <= MAX_SHARE * float(r.frame.sum()) * before.shape[0] * before.shape[1], f"{what}: too many kink pixels"
    halo = torch.ones((Hp, Wp), dtype=torch.bool)
    halo[p:p + H, p:p + W] = False
    assert bool(torch.isfinite(after).all()), f"{what}: not finite"
    assert torch.equal(after[:, :, halo], before[:, :, halo]), f"{what}: the halo was written"
    inner_a, inner_b = after[:, :, p:p + H, p:p + W], before[:, :, p:p + H, p:p + W]
    assert torch.equal(inner_a[:, :, ~r.frame], inner_b[:, :, ~r.frame]), f"{what}: a pixel outside the frame was changed"
    w1 = compare(torch.where(r.kink, r.dz, inner_a), r.dz, r.tol, what + " dz")
    w2 = compare(sums, r.sums, r.sums_tol, what + " partials")
    return w1, w2


# =============================================================================================================================
# bicubic
# =============================================================================================================================
@functools.lru_cache(maxsize=None)
def tables(n_in, n_out):
    """(idx [n_out][4], w [n_out][4] f32, start [n_in + 1], tj, tw f32) of engine.bicubic_tables."""
    return bicubic_tables(n_in, n_out)


def max_taps(n_in, n_out):
    return int(np.diff(tables(n_in, n_out)[2]).max())


@functools.lru_cache(maxsize=None)
def dense_fwd(n_in, n_out, mutant=None):
    """(T, |T|) [n_out][n_in] f64 from the forward table; taps clamped onto one input index merge (their magnitudes in the twin)."""
    idx, w = tables(n_in, n_out)[:2]
    T, A = torch.zeros((n_out, n_in), dtype=f64), torch.zeros((n_out, n_in), dtype=f64)
    for o in range(n_out):
        for k in range(4):
            i = int(idx[o, k])
            if mutant == "drop_merged" and o == n_out - 1 and k == 3 and i == int(idx[o, 2]):
                continue                                          # the last row's tap beyond the edge is skipped, not clamped
            T[o, i] += float(w[o, k])
            A[o, i] += abs(float(w[o, k]))
    return T, A


@functools.lru_cache(maxsize=None)
def dense_t(n_in, n_out, shift_at=None):
    """(T, |T|) [n_out][n_in] f64 from the transposed table.  shift_at = X: the smallest tap of input index X lands one output
    index further on."""
    _, _, start, tj, tw = tables(n_in, n_out)
    T = torch.zeros((n_out, n_in), dtype=f64)
    for i in range(n_in):
        for a in range(int(start[i]), int(start[i + 1])):
            T[int(tj[a]), i] = float(tw[a])
    if shift_at is not None:
        col = T[:, shift_at]
        nz = torch.nonzero(col).reshape(-1)
        o = int(nz[torch.argmin(col[nz].abs())])
        o2 = o + 1 if o + 1 < n_out else o - 1
        col[o2] += col[o]
        col[o] = 0.0
    return T, T.abs()


def resample(x, Ty, Tx):
    return torch.einsum("oh,nchw,pw->ncop", Ty, x, Tx)


def adjoint(g, Ty, Tx):
    return torch.einsum("oh,ncop,pw->nchw", Ty, g, Tx)


class Bic(NamedTuple):
    hi: int
    wi: int
    ho: int
    wo: int
    n: int = N
    c: int = C
    dt: str = "f32"

    @property
    def tag(self):
        return f"{self.hi}x{self.wi}->{self.ho}x{self.wo} N{self.n} c{self.c} {self.dt}"


# ---- forward ----------------------------------------------------------------------------------------------------------------
FWD_DOWN = [Bic(24, 40, 12, 20), Bic(31, 50, 16, 27), Bic(10, 40, 20, 20), Bic(24, 40, 12, 20, dt="bf16"), Bic(31, 50, 16, 27, dt="f16")]
FWD_LONG = Bic(64, 12, 128, 24, 8, 256, "bf16")
FWD_OLD = [Bic(253, 256, 506, 512, N, 8, "f16"), Bic(126, 128, 253, 256, N, 16, "bf16"), Bic(31, 32, 63, 64, N, 24), Bic(40, 300, 80, 600, N, 8),
           Bic(20, 24, 60, 72, N, 8), Bic(30, 63, 60, 127, N, 8, "f16"), Bic(5, 6, 10, 12, N, 8), Bic(7, 9, 7, 9, N, 8),
           Bic(8, 32, 128, 506, N, 8)]                                   # the shapes of test_bicubic_forward_kernel_vs_torch
FWD_ACT = [Bic(20, 24, 60, 72, dt=d) for d in ("f32", "bf16", "f16")]
FOH, FOW, FWH, FWW = 16, 64, 12, 36                                     # tile and window of k_bicubic_fwd


def fwd_takes_walk(b):
    return b.ho >= b.hi and b.wo >= b.wi


def fwd_walk_launch(b):
    """(SW, fw, strips, chunks, rpc) of mc_bicubic_fwd_act's row walk, restated."""
    SW = 128 if b.wo <= 128 else (256 if b.wo <= 256 else 512)
    fw = b.wo if b.wo <= SW else SW - 8
    strips = cdiv(b.wo, fw)
    chunks = max(1, min(cdiv(1024, cdiv(b.c, 8) * b.n * strips), cdiv(b.ho, 8)))
    return SW, fw, strips, chunks, cdiv(b.ho, chunks)


@functools.lru_cache(maxsize=None)
def fwd_input(b):
    """[N, C8 * 8, hi, wi] in the storage type, lanes past c zero."""
    return from_cb8(to_cb8(randn((b.n, b.c, b.hi, b.wi), 81 + b.hi * 1000 + b.wo, b.dt)))


@functools.lru_cache(maxsize=None)
def fwd_ref(b):
    x = fwd_input(b)
    (Ty, Ay), (Tx, Ax) = dense_fwd(b.hi, b.ho), dense_fwd(b.wi, b.wo)
    ref = resample(x, Ty, Tx)
    return ref, store_bound(gamma(K_FWD) * resample(x.abs(), Ay, Ax), ref, b.dt)


def check_fwd(b, got, what=None):
    """got [N, C8 * 8, ho, wo]; the lanes past c are exactly zero (their bound is)."""
    ref, tol = fwd_ref(b)
    return compare(got, ref, tol, what or ("bicubic forward " + b.tag))


@functools.lru_cache(maxsize=None)
def fwd_act_inputs(b, with_coef):
    x = from_cb8(to_cb8(randn((b.n, b.c, b.hi, b.wi), 91 + b.hi, b.dt, scale=1.2, shift=0.2)))
    coef = None
    if with_coef:
        g = torch.Generator().manual_seed(92)
        cp = x.shape[1]
        coef = rq(torch.stack([0.8 + 0.4 * torch.rand((b.n, cp), generator=g, dtype=f64), 0.3 * torch.randn((b.n, cp), generator=g, dtype=f64),
                               torch.zeros((b.n, cp), dtype=f64), torch.ones((b.n, cp), dtype=f64)], -1), "f32")
    return x, coef


@functools.lru_cache(maxsize=None)
def fwd_act_ref(b, act, with_coef):
    """The affine and the activation, rounded to the storage type as the staged window is, then the interpolation."""
    x, coef = fwd_act_inputs(b, with_coef)
    n, cp = x.shape[:2]
    sc = coef[:, :, 0].view(n, cp, 1, 1) if with_coef else torch.ones((n, cp, 1, 1), dtype=f64)
    sh = coef[:, :, 1].view(n, cp, 1, 1) if with_coef else torch.zeros((n, cp, 1, 1), dtype=f64)
    z, A = x * sc + sh, (x * sc).abs() + sh.abs()
    a = G.act64(z, act)
    Ea = G.LIP[act] * 2 * U * A + G.act_error(z, a, act, "f32" if b.dt == "f32" else "bf16")
    u = UNIT[DT[b.dt]]
    staged = Ea + u * (2 * a.abs() + Ea) + (2 * F16_HALF_SPACING if b.dt == "f16" else 0.0)
    aq = rq(a, b.dt)
    (Ty, Ay), (Tx, Ax) = dense_fwd(b.hi, b.ho), dense_fwd(b.wi, b.wo)
    ref = resample(aq, Ty, Tx)
    E = resample(staged, Ay, Ax) + gamma(K_FWD) * resample(aq.abs() + staged, Ay, Ax)
    return ref, store_bound(E, ref, b.dt)


def check_fwd_act(b, act, with_coef, got):
    ref, tol = fwd_act_ref(b, act, with_coef)
    return compare(got, ref, tol, f"bicubic forward with {act}{' and coef' if with_coef else ''} " + b.tag)


# ---- adjoint ----------------------------------------------------------------------------------------------------------------
ADJ_SOURCES = [Src("plain"), Src("padfold", 1), Src("padfold", 2), Src("padfold", 2, sliced=True)]     # the slice: c8_total = C8 + 2, cb_off = 1
WALK_CASES = [Bic(10, 100, 13, 128), Bic(10, 65, 20, 128), Bic(10, 200, 13, 256), Bic(30, 63, 60, 127), Bic(10, 100, 13, 128, dt="bf16"),
              Bic(30, 63, 60, 127, dt="bf16")]
WALK_LONG = Bic(64, 12, 128, 24, 8, 256, "bf16")
TAPS_CASES = [Bic(30, 30, 60, 60), Bic(30, 63, 60, 127), Bic(63, 30, 127, 60), Bic(20, 24, 60, 72), Bic(30, 63, 60, 127, dt="bf16"),
              Bic(20, 24, 60, 72, dt="bf16")]
TAPS_PERSISTENT = Bic(80, 96, 160, 192, 8, 64, "bf16")
TAPS_GATHER = Bic(8, 8, 32, 32)
TAPS_PLAIN = Bic(20, 24, 60, 72)                                       # mc_bicubic_bwd (max_taps 0, 0)
SEP_CASES = [Bic(5, 7, 20, 28), Bic(8, 8, 64, 64), Bic(8, 32, 128, 506), Bic(5, 7, 20, 28, dt="bf16"), Bic(8, 8, 64, 64, dt="bf16"),
             Bic(8, 32, 128, 506, dt="bf16")]
AGREE_CASE = Bic(20, 24, 60, 72)                                       # walk, taps and separable all accept it
BT, BWIN = 16, 40                                                      # tile and window of k_bicubic_bwd


def walk_launch(b):
    """(SW, cw, strips, chunks, rpc, BXT) of mc_bicubic_bwd_walk, restated."""
    SW = 128 if b.wo <= 128 else (256 if b.wo <= 256 else 512)
    cw, strips = b.wi, 1
    if b.wo > SW or b.wi > SW // 2:
        cw = min(SW // 2, (SW - 1) * b.wi // b.wo - 3)
        strips = cdiv(b.wi, cw)
    chunks = max(1, min(cdiv(1024, cdiv(b.c, 8) * b.n * strips), cdiv(b.hi, 4)))
    return SW, cw, strips, chunks, cdiv(b.hi, chunks), (8 if max_taps(b.wi, b.wo) <= 8 else 12)


def taps_launch(b):
    """(tiles, grid, BYT, BXT) of mc_bicubic_bwd_taps called with the case's max_taps, restated."""
    tiles = cdiv(b.wi, BT) * cdiv(b.hi, BT)
    want = max(1, (256 * 6) // max(1, cdiv(b.c, 8) * b.n))
    return tiles, min(tiles, want), (8 if max_taps(b.hi, b.ho) <= 8 else 12), (8 if max_taps(b.wi, b.wo) <= 8 else 12)


def k_adjoint(b, kernel):
    ny, nx = max_taps(b.hi, b.ho), max_taps(b.wi, b.wo)
    if kernel == "walk":
        return 2 * (ny + nx) + 3
    if kernel == "separable":
        return 2 * (ny + nx)
    return max(2 * (ny + nx), ny * nx + 1)


@functools.lru_cache(maxsize=None)
def adj_input(b):
    """The output-domain gradient [N, C8 * 8, ho, wo] in the gradient type (every lane holds data: the kernels treat all eight alike)."""
    return randn((b.n, cdiv(b.c, 8) * 8, b.ho, b.wo), 101 + b.hi * 1000 + b.wo, b.dt)


@functools.lru_cache(maxsize=4)
def adj_ref(b, kernel):
    g = adj_input(b)
    Ty, Ay = dense_fwd(b.hi, b.ho) if kernel == "walk" else dense_t(b.hi, b.ho)
    Tx, Ax = dense_t(b.wi, b.wo)
    ref = adjoint(g, Ty, Tx)
    return ref, store_bound(gamma(k_adjoint(b, kernel)) * adjoint(g.abs(), Ay, Ax), ref, b.dt)


def check_adjoint(b, kernel, got, what=None):
    """got [N, C8 * 8, hi, wi] of mc_bicubic_bwd_walk / _taps / _separable (kernel: walk | taps | separable)."""
    ref, tol = adj_ref(b, kernel)
    return compare(got, ref, tol, what or f"bicubic adjoint ({kernel}) " + b.tag)


def old_adjoint_comparison_passes(got, ref, dt):
    """The comparison of test_hip_parity.test_bicubic_adjoint_kernels_vs_torch: rtol = atol / max |ref| = 8e-3 (bf16), 2e-5 (f32)."""
    tol = 8e-3 if dt == "bf16" else 2e-5
    try:
        torch.testing.assert_close(got.float(), ref.float(), rtol=tol, atol=tol * float(ref.float().abs().max()))
    except AssertionError:
        return False
    return True


# ---- mutants of the adjoint (each returns what the mutated kernel would store) ---------------------------------------------------
def adj_mutant(b, kernel, mutant, launch=None):
    g = adj_input(b)
    Ty = (dense_fwd(b.hi, b.ho) if kernel == "walk" else dense_t(b.hi, b.ho))[0]
    Tx = dense_t(b.wi, b.wo)[0]
    if mutant == "drop_merged":                       # a clamped border row's merged weight is dropped
        Ty = dense_fwd(b.hi, b.ho, "drop_merged")[0]
    elif mutant == "seam_tap":                        # one x tap of the first column of the second strip lands one column on
        Tx = dense_t(b.wi, b.wo, walk_launch(b)[1])[0]
    elif mutant in ("no_pad_offset", "no_cb_off"):
        src = Src("padfold", 2, sliced=mutant == "no_cb_off")
        buf, tot, off = src_buffer(g, src)
        if mutant == "no_pad_offset":                 # the PADFOLD source read as if it were plain: the window starts in the halo
            g = from_cb8(buf[:, :, :b.ho, :b.wo])
        else:                                         # block cb of the wide tensor instead of cb + cb_off
            g = from_cb8(buf[:, :g.shape[1] // 8, 2:2 + b.ho, 2:2 + b.wo])
    elif mutant == "stale_origin":
        return rq(stale_origin(b, g, Ty, Tx, launch), b.dt)
    else:
        raise ValueError(mutant)
    return rq(adjoint(g, Ty, Tx), b.dt)


def stale_origin(b, g, Ty, Tx, launch=None):
    """k_bicubic_bwd whose second tile of a persistent block stages its window at the FIRST tile's origin: the tap lists index the
    window relative to the new origin, so the tile sees the gradient displaced by the difference of the two origins."""
    tiles, grid = taps_launch(launch or b)[:2]
    assert tiles > grid
    tx_n = cdiv(b.wi, BT)
    sy, jy = tables(b.hi, b.ho)[2:4]
    sx, jx = tables(b.wi, b.wo)[2:4]
    out = adjoint(g, Ty, Tx)
    for t in range(grid, tiles):
        (ty0, tx0), (py0, px0) = ((t // tx_n) * BT, (t % tx_n) * BT), (((t - grid) // tx_n) * BT, ((t - grid) % tx_n) * BT)
        dy, dx = int(jy[sy[ty0]]) - int(jy[sy[py0]]), int(jx[sx[tx0]]) - int(jx[sx[px0]])
        moved = adjoint(torch.roll(g, (dy, dx), (2, 3)), Ty, Tx)
        out[:, :, ty0:ty0 + BT, tx0:tx0 + BT] = moved[:, :, ty0:ty0 + BT, tx0:tx0 + BT]
    return out

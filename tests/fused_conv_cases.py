"""Case tables, f64 references and the derived tolerances of tests/test_hip_fused_conv.py: the fused convolution launches.
Nothing here touches a device.

Table A (EPI_CASES): the input-gradient launch with the GroupNorm-backward epilogue (mc_conv2d_fused + mc_conv_epilogue, the
FUSE == 2 instantiations of the three conv families) followed by mc_fold_padded_dz.  A case is a layer conv(c -> co, k, pad
mode) on hs x ws, the launch's precision and the activation; next to it stands the instantiation the launch must reach
(mc_conv_fused_kernel_name: the host-only name test fails when a dispatch change moves a case).

  setting   launch   y      gradients   act'
  f32       f32      f32    f32         erff / libm forms
  bf16      bf16     bf16   bf16        GELU: the f32 polynomial (GELU_GRAD_COEF); other activations: libm forms
  mixed     bf16     f16    bf16        the same, but on the row-reuse kernel with GELU and co <= 16 the packed-f16 polynomial
                                        on the MFMA waves (DZM, `,dzm`); every other row-reuse launch is the LEX form

Geometry.  p = k // 2, fr = 0 for zero padding and p + 1 otherwise.  The launch runs on the padded domain (hs + 2 p) x
(ws + 2 p); the FINAL region, padded coordinates [p + fr, p + hs - fr) x [p + fr, p + ws - fr), is stored as dz = dA act'(z),
every other pixel as raw dA; mc_fold_padded_dz then folds the halo onto the frame (the interior pixels that are not final) and
turns the frame into dz.

Reference, f64, from the stored (rounded) operands: dA = conv_transpose2d(dY, w); z = scale y + shift; dz = fold(dA) act'(z);
S1 = sum dz, S2 = sum dz (y - mean) rstd per (n, c).  For the final pixels of a DZM case act' is the kernel's own polynomial
of the clamped z = f16(scale) y + f16(shift), evaluated in f64 (dzm_model); how far that polynomial is from GELU' is measured
separately (dzm_vs_erf).

Bounds (first order in 2^-24 = E32 unless a term says otherwise; every term is written where it is added):
  E_dA       (K + 1) E32 conv_transpose2d(|dY|, |w|), K = k k co: conv_variants.tolerance's accumulation term
  raw dA     E_dA + u (|dA| + E_dA), u the unit roundoff of the stored gradient type
  E_g        f32 evaluation: LIP2 2 E32 (|scale y| + |shift|) for the rounding of z, plus gn_cases.act_grad_error (libm forms:
             (LIBM_ULP + 4) E32 LIP; the f32 polynomial: its measured error gelu_poly_errors()["E_grad"]).
             DZM: half an ulp of every f16 intermediate of the chain, propagated (dzm_model).
  dz         pre = |g| E_dA + (|dA| + E_dA) E_g + E32 |dz|  (the last term: the f32 product), then the store:
             tol = pre + u (|dz| + pre)
  frame      the fold adds cnt stored values in f32: E_fold = fold(raw-dA bound) + (cnt - 1) E32 fold(|dA| + raw-dA bound) takes
             the place of E_dA
  S1         sum of pre + (M + 1) E32 sum (|dz| + pre), M = hs ws (conv_variants.stats_ref's form: f32 partial sums in any
             order, the partials added in f64)
  S2         the same with the per-pixel bound pre |yhat| + 3 E32 |dz yhat| (yhat and the product are three f32 roundings).
             DZM forms it as rstd (sum dA hy - mean sum dz), hy = f16(g y): per pixel
             E_dA |g y| + (|dA| + E_dA) (|y| E_g + 2^-11 (|g| + E_g) |y| + 2^-24) + E32 |dA g y|, summed like S1, then
             rstd (E_sy + |mean| E_sd) + 3 E32 rstd (sum |dz y| + |mean| sum |dz|)
No element is left out of any comparison."""
import ctypes as C
import functools
import os
import re
import zlib
from typing import NamedTuple, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_variants as V
import glue_cases as Gl
import gn_cases as G
from pbml_mantle_convection_amd import _lib as L

E32 = 2.0 ** -24
DT = {"f32": "f32", "bf16": "bf16", "mixed": "mix16"}          # setting -> conv_variants' precision key
P = C.c_void_p(64)                                            # any non-null pointer for the host-only queries


def seed_of(cid):
    """A case's seed follows from its id alone: adding a case leaves the operands of the others as they are."""
    return zlib.crc32(cid.encode())


def direct(args):
    return f"k_conv_direct_f32<{args}>"


# ---- Table A ------------------------------------------------------------------------------------------------------------
class EpiCase(NamedTuple):
    id: str
    kernel: str                       # what mc_conv_fused_kernel_name must answer for the input-gradient launch
    prec: str                         # "f32" | "bf16" | "mixed"
    c: int                            # channels of the tensor the gradient belongs to (the layer's input)
    co: int                           # the layer's output channels = the launch's input channels
    k: int
    mode: str
    hw: Tuple[int, int]               # hs, ws
    groups: int
    act: str = "gelu"
    coef: bool = True                 # False: activation-only layer (no coefficient table)
    n: int = 2
    stiff: bool = False               # group 0 of every sample has |mean| rstd = 8


def _wide(cid, args, *rest, **kw):
    """A wide-tile case twice: bf16 y and f16 y."""
    return [EpiCase(cid + "-bf16", V.mf(args + ",dz"), "bf16", *rest, **kw),
            EpiCase(cid + "-mixed", V.mf(args + ",dz,h16"), "mixed", *rest, **kw)]


NT1_5, NT1_3 = "5,16,32,1,8,false", "3,16,32,1,8,false"
R8_5, NT2_3 = "5,8,16,2,2,false", "3,16,16,2,4,false"
LEX, DZM = "k_conv_rr_bf16<%d,dz%s>", "k_conv_rr_bf16<%d,dz,h16,dzm>"

EPI_CASES = [
    # ---- k_conv_direct_f32 (16 x 16 tiles)
    EpiCase("f32-k5-tile+1", direct("5,dz"), "f32", 10, 12, 5, "reflect", (13, 13), 5),
    EpiCase("f32-k3-2tile-1", direct("3,dz"), "f32", 12, 20, 3, "replicate", (29, 29), 3, act="silu"),
    EpiCase("f32-k5-nofinal", direct("5,dz"), "f32", 16, 16, 5, "reflect", (6, 6), 16),
    EpiCase("f32-k3-onefinal", direct("3,dz"), "f32", 8, 8, 3, "replicate", (5, 5), 1, coef=False),
    EpiCase("f32-k5-zeros", direct("5,dz"), "f32", 20, 10, 5, "zeros", (15, 21), 5),
    # ---- wide-tile: 16 x 32 with one N-tile (c <= 16), 8-row tiles (k = 5, 17 .. 32 channels, <= 40 rows), two N-tiles k = 3
    *_wide("w5-nt1-tile+1", NT1_5, 10, 20, 5, "reflect", (13, 29), 10),
    *_wide("w3-nt1-2tile-1", NT1_3, 12, 16, 3, "replicate", (29, 61), 6),
    *_wide("w5-8r-tile+1", R8_5, 20, 12, 5, "zeros", (5, 13), 5),
    *_wide("w5-8r-2tile-1", R8_5, 20, 32, 5, "reflect", (11, 27), 10),
    *_wide("w3-nt2-tile+1", NT2_3, 20, 16, 3, "reflect", (15, 15), 5, coef=False),
    *_wide("w5-nt1-nofinal", NT1_5, 16, 10, 5, "replicate", (6, 6), 2),
    *_wide("w3-nt1-onefinal", NT1_3, 16, 12, 3, "reflect", (5, 5), 4),
    # ---- row reuse (16 x 64 tiles; the padded domain is at least 140 columns wide, so that the widths "tile + 1" and
    # "2 tile - 1" of the other families become 3 x 64 + 1 and 3 x 64 - 1 here, and the cases without / with one final pixel
    # are so in their rows only).  LEX: the loader waves form dz, one stage late
    EpiCase("lex5-bf16-tile+1", LEX % (5, ""), "bf16", 10, 16, 5, "reflect", (13, 189), 5),
    EpiCase("lex3-bf16-silu-2tile-1", LEX % (3, ",act"), "bf16", 12, 12, 3, "replicate", (29, 189), 3, act="silu"),
    EpiCase("lex5-h16-co20", LEX % (5, ",h16"), "mixed", 16, 20, 5, "zeros", (20, 140), 16),
    EpiCase("lex3-h16-silu-nofinal", LEX % (3, ",act,h16"), "mixed", 20, 16, 3, "reflect", (4, 150), 5, act="silu"),
    EpiCase("lex3-h16-co24", LEX % (3, ",h16"), "mixed", 16, 24, 3, "replicate", (9, 140), 8),
    EpiCase("lex5-bf16-silu", LEX % (5, ",act"), "bf16", 12, 16, 5, "zeros", (9, 141), 6, act="silu"),
    EpiCase("lex5-h16-silu", LEX % (5, ",act,h16"), "mixed", 10, 16, 5, "reflect", (9, 150), 10, act="silu"),
    EpiCase("lex5-bf16-onefinal", LEX % (5, ""), "bf16", 16, 16, 5, "replicate", (7, 140), 2, coef=False),
    # 20 channels = 2 work-group columns -> 128 work-groups each; 3 x 3 tiles of 37 x 154, N = 15: 135 items, seven
    # work-groups walk two.  The epilogue of a work-group's last item runs after its loop
    EpiCase("lex5-bf16-persistent", LEX % (5, ""), "bf16", 20, 16, 5, "reflect", (33, 150), 5, n=15),
    EpiCase("lex3-bf16-stiff", LEX % (3, ""), "bf16", 16, 16, 3, "zeros", (18, 141), 4, stiff=True),
    # DZM: the MFMA waves form dz in packed f16.  seam: the final region [5, 32) x [5, 192) ends exactly on a tile edge: tiles
    # (1, 1) and (1, 2) take the unmasked rows(true) path, their neighbours the masked one; with hs one smaller none does
    EpiCase("dzm5-seam", DZM % 5, "mixed", 16, 16, 5, "reflect", (33, 193), 4),
    EpiCase("dzm5-seam-1", DZM % 5, "mixed", 16, 16, 5, "reflect", (32, 193), 4),
    EpiCase("dzm3-tile+1", DZM % 3, "mixed", 10, 12, 3, "replicate", (15, 191), 5),
    EpiCase("dzm3-2tile-1", DZM % 3, "mixed", 12, 10, 3, "zeros", (29, 189), 3, coef=False),
    EpiCase("dzm5-nofinal", DZM % 5, "mixed", 20, 16, 5, "replicate", (6, 140), 20),
    EpiCase("dzm3-onefinal", DZM % 3, "mixed", 16, 8, 3, "reflect", (5, 150), 2),
    EpiCase("dzm5-persistent", DZM % 5, "mixed", 20, 16, 5, "replicate", (33, 150), 10, n=15),
    # zero padding: final region [2, 32) x [2, 192), tiles (1, 1) and (1, 2) unmasked
    EpiCase("dzm5-stiff", DZM % 5, "mixed", 16, 16, 5, "zeros", (30, 190), 4, stiff=True),
]
EPI_BY_ID = {c.id: c for c in EPI_CASES}
assert len(EPI_BY_ID) == len(EPI_CASES)
EPI_IDS = [c.id for c in EPI_CASES]

# the instantiations Table A must reach
EPI_KERNELS = {
    direct("3,dz"), direct("5,dz"),
    *(V.mf(a + s) for a in (NT1_5, NT1_3, R8_5, NT2_3) for s in (",dz", ",dz,h16")),
    *(LEX % (k, s) for k in (3, 5) for s in ("", ",act", ",h16", ",act,h16")), DZM % 5, DZM % 3,
}


def is_dzm(c):
    return c.kernel.endswith(",dzm>")


def is_rr(c):
    return c.kernel.startswith("k_conv_rr_bf16")


def pad_of(c):
    return c.k // 2


def frame_of(c):
    return 0 if c.mode == "zeros" else pad_of(c) + 1


def padded_hw(c):
    return c.hw[0] + 2 * pad_of(c), c.hw[1] + 2 * pad_of(c)


def final_box(c):
    """(y0, y1, x0, x1) of the final region in padded coordinates (empty when y1 <= y0 or x1 <= x0)."""
    p, fr = pad_of(c), frame_of(c)
    return p + fr, p + c.hw[0] - fr, p + fr, p + c.hw[1] - fr


def final_mask(c):
    """[Hp, Wp] bool: the pixels the conv launch stores as dz."""
    hp, wp = padded_hw(c)
    y0, y1, x0, x1 = final_box(c)
    m = torch.zeros((hp, wp), dtype=torch.bool)
    if y1 > y0 and x1 > x0:
        m[y0:y1, x0:x1] = True
    return m


def tile_of(c):
    """(rows, columns) of the launch's output tile."""
    return V.tile_of(c.kernel)


def unmasked_tiles(c):
    """DZM: the tiles (ty, tx) that take the rows(true) path -- the kernel's condition, restated."""
    hp, wp = padded_hw(c)
    p, fr = pad_of(c), frame_of(c)
    c8 = (c.c + 7) // 8
    out = []
    for ty in range(-(-hp // 16)):
        for tx in range(-(-wp // 64)):
            ty0, tx0 = 16 * ty, 64 * tx
            if (ty0 + 16 <= hp and tx0 + 64 <= wp and c8 >= 2 and ty0 - p >= fr and ty0 - p + 16 <= c.hw[0] - fr and
                    tx0 - p >= fr and tx0 - p + 64 <= c.hw[1] - fr):
                out.append((ty, tx))
    return out


def layer(c):
    """The layer as a conv_variants.Case (descriptors through conv_variants.descs)."""
    return V.Case(c.id, "", "", (c.c,), c.co, c.k, c.mode, c.hw, n=c.n, f32=c.prec == "f32")


def epi_descs(c):
    """(layer descriptor, input-gradient descriptor)."""
    return V.descs(layer(c), DT[c.prec])


def epi_slots(c):
    """(slots the conv launch fills, slots of mc_fold_padded_dz behind them)."""
    lib = L.load()
    tiles = lib.mc_conv_tiles(C.byref(epi_descs(c)[1]))
    assert tiles > 0
    return tiles, lib.mc_fold_blocks(c.hw[0], c.hw[1], pad_of(c), L.PAD_MODES[c.mode])


def epilogue(c, y, coef, partials):
    tiles, fb = epi_slots(c)
    return L.ConvEpilogue(y, coef if c.coef else None, L.ACTS[c.act], pad_of(c), L.PAD_MODES[c.mode], c.hw[0], c.hw[1], partials,
                          tiles + fb, int(c.prec == "mixed"))


def fused_name(d, pro=None, epi=None):
    return L.load().mc_conv_fused_kernel_name(C.byref(d), C.byref(pro) if pro is not None else None,
                                              C.byref(epi) if epi is not None else None).decode()


def epi_name(c):
    return fused_name(epi_descs(c)[1], epi=epilogue(c, P, P, P))


# ---- operands -----------------------------------------------------------------------------------------------------------
class EpiOps(NamedTuple):
    y: torch.Tensor              # [n, c, hs, ws] f32, as handed to mc_pack_nchw
    dY: torch.Tensor             # [n, co, hs, ws] f32
    w: torch.Tensor              # [co, c, k, k] f32, as handed to mc_pack_weights
    coef: torch.Tensor           # [n, c8 * 8, 4] f32 = (scale, shift, mean, rstd), zero rows past c; None without a table


def coef_table(y64, groups, gamma, beta):
    """The table as mc_gn_finalize_coef forms it, from the statistics of the stored y."""
    n, c = y64.shape[:2]
    cpg = c // groups
    yg = y64.reshape(n, groups, -1)
    mean = yg.mean(-1).repeat_interleave(cpg, 1)
    rstd = (yg.var(-1, unbiased=False) + G.EPS).rsqrt().repeat_interleave(cpg, 1)
    sc = rstd * gamma.double()
    tab = torch.zeros((n, (c + 7) // 8 * 8, 4), dtype=torch.float32)
    tab[:, :c] = torch.stack([sc, beta.double() - mean * sc, mean, rstd], -1).float()
    return tab


@functools.lru_cache(maxsize=None)
def epi_operands(cid):
    c = EPI_BY_ID[cid]
    g = torch.Generator().manual_seed(seed_of(cid))
    hs, ws = c.hw
    scale = 0.5 + 1.5 * torch.rand((1, c.c, 1, 1), generator=g)
    offset = 0.7 * torch.randn((1, c.c, 1, 1), generator=g)
    y = torch.randn((c.n, c.c, hs, ws), generator=g) * scale + offset
    cpg = c.c // c.groups
    if c.stiff:                            # group 0: one offset for its channels, so that its mean is 8 standard deviations
        y0 = y[:, :cpg].double().reshape(c.n, -1)
        shift = 8.0 * y0.std(-1, unbiased=False) - y0.mean(-1)
        y[:, :cpg] = (y[:, :cpg].double() + shift.view(c.n, 1, 1, 1)).float()
    dY = torch.randn((c.n, c.co, hs, ws), generator=g)
    w = torch.randn((c.co, c.c, c.k, c.k), generator=g) / (c.c * c.k * c.k) ** 0.5
    gamma = 1.0 + 0.3 * torch.randn(c.c, generator=g)
    beta = 0.3 * torch.randn(c.c, generator=g)
    coef = coef_table(V.rnd(y, V.FWD_T[DT[c.prec]]), c.groups, gamma, beta) if c.coef else None
    return EpiOps(y, dY, w, coef)


def coef_columns(c, coef):
    """(scale, shift, mean, rstd), each [n, c, 1, 1] f64; without a table (1, 0, 0, 0), the kernels' defaults."""
    if coef is None:
        one = torch.ones((c.n, c.c, 1, 1), dtype=torch.float64)
        return one, 0 * one, 0 * one, 0 * one
    t = coef.double()[:, :c.c]
    return tuple(t[:, :, i].reshape(c.n, c.c, 1, 1) for i in range(4))


# ---- the DZM polynomial --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dzm_coefs():
    """(Q4's five coefficients, highest order first, and the clamp) of the DZM epilogue in csrc/conv_rr_bf16.hip, as the f16
    values the kernel holds: an f32 literal converted to _Float16."""
    src = open(os.path.join(G.ROOT, "pbml_mantle_convection_amd", "csrc", "conv_rr_bf16.hip")).read()
    body = src[src.index("if constexpr (DZM) {\n        // ---- input gradient"):]
    body = body[:body.index("rows(std::true_type{})")]
    vals = re.findall(r"\(h2\)\{\(_Float16\)(-?\d\.\d+e[-+]\d+)f, \(_Float16\)(-?\d\.\d+e[-+]\d+)f\}", body)
    assert len(vals) == 5 and all(a == b for a, b in vals), vals
    clamp = re.search(r"const h2 R = \{\(_Float16\)(\d\.\d+)f, \(_Float16\)(\d\.\d+)f\};", body)
    assert clamp and clamp.group(1) == clamp.group(2)
    h = lambda s: float(np.float32(float(s)).astype(np.float16))      # noqa: E731
    return tuple(h(a) for a, _ in vals), h(clamp.group(1))


def f16(x):
    """x (f64) rounded to f16, as f64."""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def half_ulp16(x):
    """Half the f16 spacing in the binade of |x| (subnormals: 2^-25): the rounding error of a value of magnitude <= |x|."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 11)


class DzmG(NamedTuple):
    g16: np.ndarray              # the chain in f16 arithmetic: what the kernel computes
    g: np.ndarray                # the polynomial of the clamped z in f64: the reference
    E: np.ndarray                # running bound of the f16 roundings through the chain
    z: np.ndarray                # f16(scale) y + f16(shift), unclamped, f64


def dzm_chain(z0):
    """The chain from the exact affine value z0 on (z0 = f16(scale) y + f16(shift), or a grid of arguments)."""
    coefs, R = dzm_coefs()
    fma = lambda a, b, c: f16(a * b + c)       # noqa: E731  an f16 FMA: the product and sum are exact in f64, one rounding
    z0 = np.asarray(z0, dtype=np.float64)
    # f16 arithmetic
    z = np.clip(f16(z0), -R, R)
    w = f16(z * z)
    q = fma(np.full_like(z, coefs[0]), w, coefs[1])
    for ck in coefs[2:]:
        q = fma(q, w, ck)
    g16 = fma(z, q, 0.5)
    # f64 reference and the running bound: e_x bounds |x (f16 chain) - x (f64)|; magnitudes are taken with the bound added
    zr = np.clip(z0, -R, R)
    ez = half_ulp16(z0)                        # (the clamp is 1-Lipschitz and its ends are f16 values)
    wr = zr * zr
    ew = 2 * np.abs(zr) * ez + ez * ez
    ew = ew + half_ulp16(wr + ew)
    qr = np.full_like(zr, coefs[0])
    eq = np.zeros_like(zr)
    for ck in coefs[1:]:
        qn = qr * wr + ck
        en = np.abs(qr) * ew + (wr + ew) * eq
        eq = en + half_ulp16(np.abs(qn) + en)
        qr = qn
    gr = 0.5 + zr * qr
    eg = np.abs(zr) * eq + (np.abs(qr) + eq) * ez
    eg = eg + half_ulp16(np.abs(gr) + eg)
    return DzmG(g16, gr, eg, z0)


def dzm_model(y, sc, sh):
    """y: f64 values of an f16 tensor; sc, sh: f64 values of the f32 table (broadcastable).  The affine map runs in f16 on the
    f16-rounded coefficients (pk_f16: round to nearest even)."""
    return dzm_chain(f16(sc) * np.asarray(y, dtype=np.float64) + f16(sh))


@functools.lru_cache(maxsize=None)
def dzm_vs_erf():
    """The DZM polynomial, as the kernel evaluates it (f16 chain, scale 1, shift 0), against erf-form GELU' in f64:
    (max |error| over [-8, 8] on every f16 argument, rms error over z ~ N(0, 1))."""
    bits = np.arange(0, 0x7C00, dtype=np.uint16)                      # every finite non-negative f16
    z = bits.view(np.float16).astype(np.float64)
    z = np.concatenate([-z[::-1], z])
    z = z[np.abs(z) <= 8.0]
    z64 = torch.from_numpy(z)
    exact = 0.5 * (1.0 + torch.erf(z64 / 2.0 ** 0.5)) + z64 * torch.exp(-0.5 * z64 * z64) / (2.0 * np.pi) ** 0.5
    err = np.abs(dzm_chain(z).g16 - exact.numpy())
    # rms under the normal density: sum err^2 pdf dz over the f16 grid (trapezoid on the grid's own spacing)
    pdf = np.exp(-0.5 * z * z) / (2.0 * np.pi) ** 0.5
    dzs = np.gradient(z)
    rms = float(np.sqrt(np.sum(err * err * pdf * dzs) / np.sum(pdf * dzs)))
    return float(err.max()), rms


# ---- reference of Table A ------------------------------------------------------------------------------------------------
def act_model(c, y64, sc, sh, dzm):
    """(act'(z) reference, bound E_g on the kernel's value), both [n, c, hs, ws] f64, for an f32 evaluation (dzm False) or the
    DZM chain."""
    if dzm:
        m = dzm_model(y64.numpy(), sc.numpy(), sh.numpy())
        return torch.from_numpy(m.g), torch.from_numpy(m.E)
    z, A = y64 * sc + sh, (y64 * sc).abs() + sh.abs()
    Ez = 2 * E32 * A if c.coef else 0 * A                              # (y * 1 + 0 is exact)
    return G.act_grad64(z, c.act), G.LIP2[c.act] * Ez + G.act_grad_error(z, c.act, "f32" if c.prec == "f32" else "bf16")


class Sums(NamedTuple):
    s: torch.Tensor              # [n, c, 2] = (S1, S2)
    tol: torch.Tensor


class EpiRef(NamedTuple):
    final: torch.Tensor          # [Hp, Wp] bool
    stage1: torch.Tensor         # [n, c, Hp, Wp]: the padded buffer after the conv launch
    tol1: torch.Tensor
    sums1: Sums                  # slots 0 .. tiles - 1
    stage2: torch.Tensor         # ... after mc_fold_padded_dz
    tol2: torch.Tensor
    sums2: Sums                  # all slots


def _sum_bounds(term, E, M):
    return E.sum((2, 3)) + (M + 1) * E32 * (term.abs() + E).sum((2, 3))


def region_sums(c, mask, dA, E_dA, g, E_g, pre, y64, cols, dzm):
    """(S1, S2) over the pixels of `mask` ([hs, ws] bool) and their bounds.  dA, E_dA: the (folded) gradient and its bound on the
    interior; pre: the bound on the f32 dz."""
    _, _, me, rs = cols
    M = c.hw[0] * c.hw[1]
    mk = mask.to(torch.float64)
    dz = dA * g * mk
    pre = pre * mk
    yhat = (y64 - me) * rs
    s1, t1 = dz.sum((2, 3)), _sum_bounds(dz, pre, M)
    s2 = (dz * yhat).sum((2, 3))
    if not dzm:
        e2 = pre * yhat.abs() + 3 * E32 * (dz * yhat).abs()
        t2 = e2.sum((2, 3)) + (M + 2) * E32 * ((dz * yhat).abs() + e2).sum((2, 3))
    else:
        gy = (g * y64).abs()
        e_sy = (E_dA * gy + (dA.abs() + E_dA) * (y64.abs() * E_g + 2.0 ** -11 * (g.abs() + E_g) * y64.abs() + V.F16_SPACING)
                + E32 * dA.abs() * gy) * mk
        dzy = dz * y64
        t_sy = _sum_bounds(dzy, e_sy, M)
        r, m = rs.reshape(c.n, c.c), me.reshape(c.n, c.c).abs()
        t2 = r * (t_sy + m * t1) + 3 * E32 * r * (dzy.abs().sum((2, 3)) + m * dz.abs().sum((2, 3)))
    return Sums(torch.stack([s1, s2], -1), torch.stack([t1, t2], -1))


def epi_eval(c, ops, mutant=None):
    """The reference (mutant None) or what a kernel with `mutant` would leave, unrounded:
      "frame_p"     final region one pixel wider: frame width p instead of p + 1 (both kernels)
      "act_at_y"    act' taken at y instead of scale y + shift
      "no_mean"     mean omitted from yhat
      "next_row"    every channel reads the coefficient row of its neighbour"""
    dt = DT[c.prec]
    ft, gt = V.FWD_T[dt], V.GRAD_T[dt]
    u = V.UNIT[gt]
    p, fr = pad_of(c), frame_of(c)
    hs, ws = c.hw
    y64, dY64, w64 = V.rnd(ops.y, ft), V.rnd(ops.dY, gt), V.rnd(ops.w, gt)
    dA = F.conv_transpose2d(dY64, w64)
    S = F.conv_transpose2d(dY64.abs(), w64.abs())
    K = c.k * c.k * c.co
    E_dA = (K + 1) * E32 * S
    tol_raw = V.tolerance(dA, S, K, u)
    coef = ops.coef
    if mutant == "next_row" and coef is not None:
        coef = coef.clone()
        coef[:, :c.c] = torch.roll(ops.coef[:, :c.c], 1, 1)
    cols = list(coef_columns(c, coef))
    if mutant == "no_mean":
        cols[2] = 0 * cols[2]
    sc, sh = cols[0], cols[1]
    if mutant == "act_at_y":
        sc, sh = torch.ones_like(sc), torch.zeros_like(sh)
    if mutant == "frame_p" and fr:
        fr -= 1
    final_i = torch.zeros((hs, ws), dtype=torch.bool)
    if hs > 2 * fr and ws > 2 * fr:
        final_i[fr:hs - fr, fr:ws - fr] = True
    final = torch.zeros((hs + 2 * p, ws + 2 * p), dtype=torch.bool)
    final[p:p + hs, p:p + ws] = final_i
    inner = lambda t: t[:, :, p:p + hs, p:p + ws]          # noqa: E731

    def dz_bound(dAx, Ex, g, Eg):
        pre = g.abs() * Ex + (dAx.abs() + Ex) * Eg + E32 * (dAx * g).abs()
        return pre, pre + u * ((dAx * g).abs() + pre)

    # stage 1: the conv launch.  Final pixels: dz by the launch's own act' (DZM: the f16 polynomial)
    g1, Eg1 = act_model(c, y64, sc, sh, is_dzm(c))
    pre1, tol_dz1 = dz_bound(inner(dA), inner(E_dA), g1, Eg1)
    stage1, tol1 = dA.clone(), tol_raw.clone()
    inner(stage1)[:, :, final_i] = (inner(dA) * g1)[:, :, final_i]
    inner(tol1)[:, :, final_i] = tol_dz1[:, :, final_i]
    sums1 = region_sums(c, final_i, inner(dA), inner(E_dA), g1, Eg1, pre1, y64, cols, is_dzm(c))
    # stage 2: mc_fold_padded_dz on the frame, from the stored raw values, act' in f32
    stage2, tol2, sums2 = stage1.clone(), tol1.clone(), sums1
    if fr:
        frame_i = ~final_i
        cnt = Gl.fold_autograd(torch.ones_like(dA), p, c.mode).round()
        dAf = Gl.fold_autograd(dA, p, c.mode)
        E_fold = Gl.fold_autograd(tol_raw, p, c.mode) + (cnt - 1) * E32 * Gl.fold_autograd(dA.abs() + tol_raw, p, c.mode)
        g2, Eg2 = act_model(c, y64, sc, sh, False)
        pre2, tol_dz2 = dz_bound(dAf, E_fold, g2, Eg2)
        inner(stage2)[:, :, frame_i] = (dAf * g2)[:, :, frame_i]
        inner(tol2)[:, :, frame_i] = tol_dz2[:, :, frame_i]
        fs = region_sums(c, frame_i, dAf, E_fold, g2, Eg2, pre2, y64, cols, False)
        sums2 = Sums(sums1.s + fs.s, sums1.tol + fs.tol)
    return EpiRef(final, stage1, tol1, sums1, stage2, tol2, sums2)


@functools.lru_cache(maxsize=None)
def epi_ref(cid):
    c = EPI_BY_ID[cid]
    return epi_eval(c, epi_operands(cid))


def stored_grad(c, t):
    """t after the store to the gradient type of the case."""
    return t.to(torch.float32).to(V.GRAD_T[DT[c.prec]]).double()


# ---- Table B: mc_gn_bwd_apply_dz and mc_conv2d_wgrad_dz -------------------------------------------------------------------
# dy = scale dz - rstd (m1 + yhat m2), yhat = (y - mean) rstd, per element in f64.  The kernels form cA = scale,
# cB = -rstd rstd m2 (two roundings), cC = -rstd m1 (one), t = y - mean (one), then two FMAs: at most five f32 roundings on any
# of the three terms: E = 5 E32 (|cA dz| + |cB t| + |cC|), then the store.  Without a table dy = dz, bit for bit.
class ApplyCase(NamedTuple):
    id: str
    prec: str
    c: int
    groups: int
    hw: Tuple[int, int]
    pad: int = 0                      # 0: MC_GSRC_PLAIN; 1, 2: MC_GSRC_PADFOLD (the frame holds garbage)
    mode: str = "zeros"               # pad_mode of the gradient source
    gn: bool = True


# the launch walks 32 rows per block up to 32 columns, 16 up to 256: one block, a block + 1 row, two blocks - 1 row
APPLY_SIZES = [(32, 9), (33, 31), (31, 33)]
APPLY_SOURCES = [(0, "zeros")] + [(p, m) for p in (1, 2) for m in ("zeros", "replicate", "reflect")]
APPLY_CHANNELS = [(10, 5), (12, 3), (16, 2)]
APPLY_CASES = [ApplyCase(f"{prec}-pad{p}-{m}", prec, *APPLY_CHANNELS[(i + j) % 3], APPLY_SIZES[(i + 2 * j) % 3], p, m)
               for j, prec in enumerate(("f32", "bf16", "mixed")) for i, (p, m) in enumerate(APPLY_SOURCES)]
APPLY_CASES += [ApplyCase(f"{prec}-identity", prec, *APPLY_CHANNELS[j], APPLY_SIZES[j], 2 * (j % 2), "reflect", gn=False)
                for j, prec in enumerate(("f32", "bf16", "mixed"))]
APPLY_BY_ID = {c.id: c for c in APPLY_CASES}
assert len(APPLY_BY_ID) == len(APPLY_CASES)
APPLY_IDS = [c.id for c in APPLY_CASES]
N_B = 2


class ApplyOps(NamedTuple):
    dz: torch.Tensor             # [n, c, h, w] f32
    y: torch.Tensor
    coef: torch.Tensor           # [n, c8 * 8, 4] f32 or None
    m12: torch.Tensor            # [n, groups, 2] f32


@functools.lru_cache(maxsize=None)
def apply_operands(cid):
    c = APPLY_BY_ID[cid]
    g = torch.Generator().manual_seed(seed_of(cid))
    scale = 0.5 + 1.5 * torch.rand((1, c.c, 1, 1), generator=g)
    y = torch.randn((N_B, c.c, *c.hw), generator=g) * scale + 0.7 * torch.randn((1, c.c, 1, 1), generator=g)
    dz = torch.randn((N_B, c.c, *c.hw), generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(c.c, generator=g), 0.3 * torch.randn(c.c, generator=g)
    m12 = 0.5 * torch.randn((N_B, c.groups, 2), generator=g)
    coef = coef_table(V.rnd(y, V.FWD_T[DT[c.prec]]), c.groups, gamma, beta) if c.gn else None
    return ApplyOps(dz, y, coef, m12)


def dy_expression(dz64, y64, coef, m1, m2, E_m1=0.0, E_m2=0.0):
    """(dy, bound on the f32 value) from the table [n, c, 4] (f64) and m1, m2 [n, c, 1, 1]; E_m1, E_m2: bounds on the m12 the
    kernel was given."""
    n, c = dz64.shape[:2]
    sc, _, me, rs = (coef[:, :c, i].reshape(n, c, 1, 1) for i in range(4))
    t = y64 - me
    dy = sc * dz64 - rs * (m1 + t * rs * m2)
    E = 5 * E32 * ((sc * dz64).abs() + (rs * rs * m2 * t).abs() + (rs * m1).abs()) + rs * (E_m1 + (t * rs).abs() * E_m2)
    return dy, E


def apply_eval(c, ops, mutant=None):
    """(dy, tol).  mutant "next_group": every group reads the m1, m2 of its neighbour."""
    dt = DT[c.prec]
    gt = V.GRAD_T[dt]
    dz64, y64 = V.rnd(ops.dz, gt), V.rnd(ops.y, V.FWD_T[dt])
    if not c.gn:
        return dz64, torch.zeros_like(dz64)
    m12 = ops.m12.double()
    if mutant == "next_group":
        m12 = torch.roll(m12, 1, 1)
    cpg = c.c // c.groups
    m1, m2 = (m12[..., i].repeat_interleave(cpg, 1).reshape(N_B, c.c, 1, 1) for i in range(2))
    dy, E = dy_expression(dz64, y64, ops.coef.double(), m1, m2)
    return dy, G.store_tol(dy, E, gt) if gt != torch.float32 else E


@functools.lru_cache(maxsize=None)
def apply_ref(cid):
    return apply_eval(APPLY_BY_ID[cid], apply_operands(cid))


class WdzCase(NamedTuple):
    id: str
    ci: int
    co: int
    k: int
    mode: str                         # the layer's padding mode
    hw: Tuple[int, int]               # the layer's input = output size
    zpad: int                         # 0: dz is MC_GSRC_PLAIN; 1, 2: MC_GSRC_PADFOLD
    groups: int


# the filter-gradient kernel's work item is 16 x 32 output pixels
WDZ_CASES = [
    WdzCase("k5-16x32-plain", 16, 16, 5, "reflect", (16, 32), 0, 4),
    WdzCase("k3-17x33-zpad1", 10, 12, 3, "replicate", (17, 33), 1, 3),
    WdzCase("k5-31x63-zpad2", 10, 16, 5, "zeros", (31, 63), 2, 2),
    WdzCase("k3-31x63-plain", 16, 12, 3, "reflect", (31, 63), 0, 6),
    WdzCase("k5-small-zpad1", 16, 12, 5, "replicate", (7, 9), 1, 12),
    WdzCase("k3-small-zpad2", 10, 16, 3, "zeros", (5, 11), 2, 16),
    WdzCase("k5-17x33-zpad2", 16, 16, 5, "reflect", (17, 33), 2, 8),
]
WDZ_BY_ID = {c.id: c for c in WDZ_CASES}
assert len(WDZ_BY_ID) == len(WDZ_CASES)
WDZ_IDS = [c.id for c in WDZ_CASES]
WDZ_BLOCKS = 7                        # slots per sample of the host-made reduce partials


def wdz_layer(c):
    return V.Case(c.id, "", "", (c.ci,), c.co, c.k, c.mode, c.hw, n=N_B)


class WdzOps(NamedTuple):
    x: torch.Tensor              # [n, ci, h, w] f32
    dz: torch.Tensor             # [n, co, h, w] f32
    y: torch.Tensor              # [n, co, h, w] f32: the layer's raw conv output
    coef: torch.Tensor           # [n, co8 * 8, 4]
    gamma: torch.Tensor
    part: torch.Tensor           # [n, WDZ_BLOCKS, co8 * 8, 2] f32: (sum dz, sum dz yhat) partials, zero in padded channels


@functools.lru_cache(maxsize=None)
def wdz_operands(cid):
    c = WDZ_BY_ID[cid]
    g = torch.Generator().manual_seed(seed_of(cid))
    x = torch.randn((N_B, c.ci, *c.hw), generator=g)
    scale = 0.5 + 1.5 * torch.rand((1, c.co, 1, 1), generator=g)
    y = torch.randn((N_B, c.co, *c.hw), generator=g) * scale + 0.7 * torch.randn((1, c.co, 1, 1), generator=g)
    dz = torch.randn((N_B, c.co, *c.hw), generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(c.co, generator=g), 0.3 * torch.randn(c.co, generator=g)
    cop = (c.co + 7) // 8 * 8
    part = torch.zeros((N_B, WDZ_BLOCKS, cop, 2))
    part[:, :, :c.co] = torch.randn((N_B, WDZ_BLOCKS, c.co, 2), generator=g) * (c.hw[0] * c.hw[1] / WDZ_BLOCKS) ** 0.5
    return WdzOps(x, dz, y, coef_table(V.rnd(y, torch.float16), c.groups, gamma, beta), gamma, part)


@functools.lru_cache(maxsize=None)
def wdz_dy_ref(cid):
    """(dY, tol) of the bf16 dY the launch stores: the expression above with m12 = the group means of the gamma-weighted
    partials (gn_cases.finalize_ref, whose bound on m12 enters through E_m1, E_m2)."""
    c, ops = WDZ_BY_ID[cid], wdz_operands(cid)
    s = G.Shape(N_B, c.co, c.groups, *c.hw)
    m12, m12_tol = G.finalize_ref(ops.part[:, :, :c.co], ops.gamma, s)[:2]
    col = lambda t, i: t[..., i].repeat_interleave(s.cpg, 1).reshape(N_B, c.co, 1, 1)      # noqa: E731
    dy, E = dy_expression(V.rnd(ops.dz, torch.bfloat16), V.rnd(ops.y, torch.float16), ops.coef.double(), col(m12, 0), col(m12, 1),
                          col(m12_tol, 0) + E32 * col(m12, 0).abs(), col(m12_tol, 1) + E32 * col(m12, 1).abs())
    return dy, G.store_tol(dy, E, torch.bfloat16)


def wdz_wgrad_ref(cid, dy64):
    """(dw, tol, dbias, tol) INCLUDING the prefill, from x (f16, converted to bf16 while staged) and the dY the launch stored
    (dy64: read back): conv_variants.wgrad_ref's sums."""
    c, ops = WDZ_BY_ID[cid], wdz_operands(cid)
    lay = wdz_layer(c)
    x64 = V.rnd(ops.x, torch.float16, torch.bfloat16)

    def grads(xx, cc):
        w = torch.zeros((c.co, c.ci, c.k, c.k), dtype=torch.float64, requires_grad=True)
        b = torch.zeros((c.co,), dtype=torch.float64, requires_grad=True)
        (V.forward_eval(lay, xx, w, b) * cc).sum().backward()
        return w.grad, b.grad
    dw, db = grads(x64, dy64)
    sw, sb = grads(x64.abs(), dy64.abs())
    px = N_B * c.hw[0] * c.hw[1]
    dw, db = dw + V.WGRAD_PREFILL, db + V.WGRAD_PREFILL
    return dw, V.tolerance(dw, sw + V.WGRAD_PREFILL, px, 0.0), db, V.tolerance(db, sb + V.WGRAD_PREFILL, px, 0.0)


# ---- Table C: the normalise-on-load prologue ------------------------------------------------------------------------------
# mc_conv2d_fused with `pro` against conv(act(scale y0 + shift) | x1) in f64, and mc_conv2d_wgrad_fused the same way.  The
# activated value a is rounded to the staged type where the kernel rounds it (xform_bf16x8 / xform_f16x8; the 16-bit filter
# gradient of an MC_MIX16 layer converts the f16 value to bf16 after that) and stays unrounded in f32.  The kernel's f32 a is
# within E_a = LIP 2 E32 (|scale y| + |shift|) + gn_cases.act_error of the reference; rounding is monotone, so the value the
# kernel stages lies between the roundings of a - E_a and a + E_a: E_x = the larger distance of those two from the rounded
# reference (0 for almost every element: the interval holds no rounding boundary).  X = conv(E_x, |w|) enters the
# accumulation term's S and is added once more for itself.
class ProCase(NamedTuple):
    id: str
    kernel: str                       # forward instantiation without ",h16" (the MC_MIX16 run appends it)
    ci: Tuple[int, ...]
    co: int
    k: int
    mode: str
    hw: Tuple[int, int]
    acts: Tuple[str, str]
    coefs: Tuple[bool, bool]          # coefficient table on source 0 / 1
    groups: Tuple[int, int] = (1, 1)
    f32: bool = False


R5N, R3N = "k_conv_rr_bf16<5,norm>", "k_conv_rr_bf16<3,norm>"
PRO_CASES = [
    # ---- k_conv_direct_f32 (16 x 16 tiles)
    ProCase("f32-k5-tile+1-pair", direct("5,norm"), (8, 12), 20, 5, "reflect", (17, 17), ("gelu", "none"), (True, False), (2, 1), True),
    ProCase("f32-k3-2tile-1-silu", direct("3,norm"), (11,), 16, 3, "zeros", (31, 31), ("silu", "none"), (True, False), (11, 1), True),
    ProCase("f32-k5-min-reflect-both", direct("5,norm"), (16, 8), 4, 5, "reflect", (3, 3), ("gelu", "gelu"), (True, True), (4, 8), True),
    ProCase("f32-k3-small-act", direct("3,norm"), (16,), 16, 3, "replicate", (5, 7), ("gelu", "none"), (False, False), f32=True),
    # ---- wide-tile: two output tiles; 8-row tiles for k = 5 up to 40 rows, 16 x 16 for k = 3; one and two co-tiles per
    # filter-gradient block follow from the output tile count (32 channels: two; 48: one)
    ProCase("w5-8r-tile+1-pair", V.mf("5,8,16,2,2,false,norm"), (16, 8), 32, 5, "zeros", (9, 17), ("gelu", "none"), (True, False), (4, 1)),
    ProCase("w5-8r-2tile-1", V.mf("5,8,16,2,2,false,norm"), (11,), 32, 5, "reflect", (15, 31), ("gelu", "none"), (True, False), (11, 1)),
    ProCase("w3-nt2-tile+1-both", V.mf("3,16,16,2,4,false,norm"), (8, 12), 32, 3, "replicate", (17, 17), ("gelu", "gelu"), (True, True), (2, 3)),
    ProCase("w3-nt2-small-act", V.mf("3,16,16,2,4,false,norm"), (16,), 20, 3, "zeros", (5, 7), ("silu", "none"), (False, False)),
    ProCase("w5-8r-min-reflect", V.mf("5,8,16,2,2,false,norm"), (16,), 32, 5, "reflect", (3, 3), ("gelu", "none"), (True, False), (4, 1)),
    # ---- row reuse (16 x 64 tiles): GELU-only build, and the generic-activation build (",act")
    ProCase("rr5-tile+1-pair", R5N, (16, 8), 16, 5, "zeros", (17, 65), ("gelu", "none"), (True, False), (2, 1)),
    ProCase("rr3-2tile-1-silu", "k_conv_rr_bf16<3,norm,act>", (11,), 16, 3, "replicate", (31, 127), ("silu", "none"), (True, False), (11, 1)),
    ProCase("rr3-small-both", R3N, (8, 12), 4, 3, "zeros", (5, 9), ("gelu", "gelu"), (True, True), (1, 6)),
    ProCase("rr5-min-reflect-act", R5N, (16,), 16, 5, "reflect", (3, 3), ("gelu", "none"), (False, False)),
    ProCase("rr5-3tiles-mixed-acts", "k_conv_rr_bf16<5,norm,act>", (16, 8), 48, 5, "zeros", (17, 65), ("gelu", "silu"), (True, True), (8, 2)),
]
PRO_BY_ID = {c.id: c for c in PRO_CASES}
assert len(PRO_BY_ID) == len(PRO_CASES)
PRO_RUNS = [(c.id, dt) for c in PRO_CASES for dt in (("f32",) if c.f32 else ("bf16", "mix16"))]
PRO_RUN_IDS = [f"{i}-{dt}" for i, dt in PRO_RUNS]
# the instantiations Table C must reach (a 16-bit case runs as MC_BF16 and as MC_MIX16: ",h16")
PRO_KERNELS = {
    direct("3,norm"), direct("5,norm"),
    *(V.mf(a + ",norm" + h) for a in (R8_5, NT2_3) for h in ("", ",h16")),
    *(f"k_conv_rr_bf16<{k},norm{a}{h}>" for k in (3, 5) for a in ("", ",act") for h in ("", ",h16")),
}


def pro_layer(c):
    return V.Case(c.id, "", "", c.ci, c.co, c.k, c.mode, c.hw, n=N_B, f32=c.f32)


def prologue(c, coef0, coef1):
    return L.ConvPrologue(coef0 if c.coefs[0] else None, coef1 if c.coefs[1] else None, L.ACTS[c.acts[0]], L.ACTS[c.acts[1]])


def pro_name(c, dt):
    return fused_name(V.descs(pro_layer(c), dt)[0], pro=prologue(c, P, P))


class ProOps(NamedTuple):
    src: Tuple[torch.Tensor, ...]        # the one or two sources, f32 [n, ci_k, h, w]
    coef: Tuple[object, ...]             # per source and precision key: {dt: table or None}
    w: torch.Tensor
    b: torch.Tensor
    ct: torch.Tensor                     # cotangent [n, co, h, w]


@functools.lru_cache(maxsize=None)
def pro_operands(cid):
    c = PRO_BY_ID[cid]
    g = torch.Generator().manual_seed(seed_of(cid))
    src, coef = [], []
    for k, ci in enumerate(c.ci):
        scale = 0.5 + 1.5 * torch.rand((1, ci, 1, 1), generator=g)
        x = torch.randn((N_B, ci, *c.hw), generator=g) * scale + 0.7 * torch.randn((1, ci, 1, 1), generator=g)
        gamma, beta = 1.0 + 0.3 * torch.randn(ci, generator=g), 0.3 * torch.randn(ci, generator=g)
        src.append(x)
        # (the table follows the statistics of the stored tensor, which differ by precision)
        coef.append({dt: coef_table(V.rnd(x, V.FWD_T[dt]), c.groups[k], gamma, beta) if c.coefs[k] else None
                     for dt in (("f32",) if c.f32 else ("bf16", "mix16"))})
    cin = sum(c.ci)
    w = torch.randn((c.co, cin, c.k, c.k), generator=g) / (cin * c.k * c.k) ** 0.5
    b = 0.1 * torch.randn((c.co,), generator=g)
    ct = torch.randn((N_B, c.co, *c.hw), generator=g)
    return ProOps(tuple(src), tuple(coef), w, b, ct)


def staged_sources(c, dt, stage, mutant=None):
    """(x, E_x, pad value per channel): the concatenated sources as the kernel stages them, in f64; `stage`: the types the
    activated value is rounded through (empty: f32, unrounded).  The third result is act(shift) per (n, channel, 1, 1) where a
    source is transformed and 0 elsewhere: what the "pad_act" mutant leaves in zero-padded pixels."""
    ops = pro_operands(c.id)
    xs, es, ps = [], [], []
    for k, ci in enumerate(c.ci):
        x64 = V.rnd(ops.src[k], V.FWD_T[dt])
        act, tab = c.acts[k], ops.coef[k][dt]
        if act == "none" and tab is None:
            xs.append(x64), es.append(torch.zeros_like(x64)), ps.append(torch.zeros((N_B, ci, 1, 1), dtype=torch.float64))
            continue
        one = torch.ones((N_B, ci, 1, 1), dtype=torch.float64)
        sc, sh = (tab.double()[:, :ci, i].reshape(N_B, ci, 1, 1) for i in range(2)) if tab is not None else (one, 0 * one)
        z, A = x64 * sc + sh, (x64 * sc).abs() + sh.abs()
        a = G.act64(z, act)
        Ea = G.LIP[act] * (2 * E32 * A if tab is not None else 0 * A) + G.act_error(z, a, act, "f32" if dt == "f32" else "bf16")
        if stage:
            r, lo, hi = V.rnd(a, *stage), V.rnd(a - Ea, *stage), V.rnd(a + Ea, *stage)
            xs.append(r), es.append(torch.maximum((hi - r).abs(), (lo - r).abs()))
        else:
            xs.append(a), es.append(Ea)
        ps.append(G.act64(sh, act) if stage == () else V.rnd(G.act64(sh, act), *stage))
    return torch.cat(xs, 1), torch.cat(es, 1), torch.cat(ps, 1)


@functools.lru_cache(maxsize=None)
def pro_forward_ref(cid, dt, mutant=None):
    """(y, tol) of mc_conv2d_fused with the prologue.  mutant "pad_act": the zero-padded pixels hold act(shift)."""
    c, ops = PRO_BY_ID[cid], pro_operands(cid)
    lay = pro_layer(c)
    ft = V.FWD_T[dt]
    x, Ex, padv = staged_sources(c, dt, () if dt == "f32" else (ft,))
    w64, b64 = V.rnd(ops.w, ft), ops.b.double()
    if mutant == "pad_act":
        assert c.mode == "zeros"
        p = c.k // 2
        xp = padv.expand(-1, -1, c.hw[0] + 2 * p, c.hw[1] + 2 * p).clone()
        xp[:, :, p:p + c.hw[0], p:p + c.hw[1]] = x
        return F.conv2d(xp, w64, b64), None
    y = V.forward_eval(lay, x, w64, b64)
    S = V.forward_eval(lay, x.abs(), w64.abs(), b64.abs())
    X = V.forward_eval(lay, Ex, w64.abs(), 0 * b64)
    K = c.k * c.k * sum(c.ci)
    u = V.UNIT[ft]
    return y, V.tolerance(y, S + X, K, u, V.F16_SPACING if ft == torch.float16 else 0.0) + (1 + u) * X


@functools.lru_cache(maxsize=None)
def pro_wgrad_ref(cid, dt):
    """(dw, tol, dbias, tol) INCLUDING the prefill of mc_conv2d_wgrad_fused + mc_conv2d_wgrad_finalize: conv_variants.wgrad_ref's
    sums over the staged sources (MC_MIX16: f16, then bf16) and the cotangent in the gradient type."""
    c, ops = PRO_BY_ID[cid], pro_operands(cid)
    lay = pro_layer(c)
    stage = {"f32": (), "bf16": (torch.bfloat16,), "mix16": (torch.float16, torch.bfloat16)}[dt]
    x, Ex, _ = staged_sources(c, dt, stage)
    if dt == "mix16":                                   # (an untransformed f16 source is converted to bf16 all the same)
        x = V.rnd(x, torch.bfloat16)
    ct64 = V.rnd(ops.ct, V.GRAD_T[dt])

    def grads(xx, cc):
        w = torch.zeros(ops.w.shape, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(ops.b.shape, dtype=torch.float64, requires_grad=True)
        (V.forward_eval(lay, xx, w, b) * cc).sum().backward()
        return w.grad, b.grad
    dw, db = grads(x, ct64)
    sw, sb = grads(x.abs(), ct64.abs())
    Xw = grads(Ex, ct64.abs())[0]
    px = N_B * c.hw[0] * c.hw[1]
    dw, db = dw + V.WGRAD_PREFILL, db + V.WGRAD_PREFILL
    return dw, V.tolerance(dw, sw + Xw + V.WGRAD_PREFILL, px, 0.0) + Xw, db, V.tolerance(db, sb + V.WGRAD_PREFILL, px, 0.0)

"""Case table, f64 references and the derived tolerance of tests/test_hip_conv_variants.py.

Every case is one convolution LAYER ('same'-style descriptor as the engine builds it, engine._conv_descs): its forward launch,
the input-gradient launch on the padded domain and the filter gradient.  Next to each case stands the kernel instantiation
its forward and its input-gradient descriptor must reach (mc_conv_kernel_name); the host-only name test fails when a dispatch
change moves a case to another variant.  Nothing here touches a device."""
import ctypes as C
import functools
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from pbml_mantle_convection_amd import _lib as L


def mf(args):
    return f"k_conv_mfma_bf16<{args}>"


def rr(args):
    return f"k_conv_rr_bf16<{args}>"


def direct(k):
    return f"k_conv_direct_f32<{k}>"


NT1_5, NT1_3 = mf("5,16,32,1,8,false"), mf("3,16,32,1,8,false")


class Case(NamedTuple):
    id: str
    fwd: str                          # kernel of the forward descriptor
    dgrad: str                        # kernel of the input-gradient descriptor
    ci: Tuple[int, ...]               # channels of the one or two concatenated sources
    co: int
    k: int
    mode: str
    hw: Tuple[int, int]               # INPUT size; the output is (h + 2 pad - k + 1) x (w + 2 pad - k + 1)
    sym: Tuple[int, int, int] = (0, 0, 0)     # (sym_h, sym_v, sym_hv)
    n: int = 2
    pad: int = -1                     # -1: k // 2
    out_f32: int = 0
    f32: bool = False                 # MC_F32 case (else the case runs as MC_BF16 and again as MC_MIX16)


# Tile shapes: f32 direct 16 x 16; wide-tile TH x 16 (TH = 8 / 12 / 16 / 24 by cfg_for) or 16 x 32 with one N-tile; row reuse
# 16 x 64 in four 16-column strips.  Per family at least one case with Ho, Wo = tile + 1, one with 2 tile - 1 and one smaller
# than a tile in both axes; padded width of the input gradient = W + 2 pad (row reuse from 140, else wide-tile).
CASES = [
    # ---- wide-tile, k = 5, forward: even number of 16-channel output tiles, Wo < 100; TH from cfg_for(c_out, 5, Ho)
    Case("w5-8r-nt2-tile+1", mf("5,8,16,2,2,false"), NT1_5, (11,), 32, 5, "reflect", (9, 17), (8, 0, 0)),
    Case("w5-8r-nt2-min-reflect", mf("5,8,16,2,2,false"), NT1_5, (16,), 20, 5, "reflect", (3, 3), (4, 0, 0)),
    # input gradient: 24 channels = 2 N-tiles on 19 x 35 -> 8-row tiles, split at 16
    Case("w5-8r-nt4-2tile-1", mf("5,8,16,4,4,false,2x2"), mf("5,8,16,2,2,false"), (16, 8), 64, 5, "replicate", (15, 31), (16, 0, 0)),
    Case("w5-16r-nt2", mf("5,16,16,2,4,false"), NT1_5, (48,), 32, 5, "zeros", (47, 17), (8, 0, 0)),
    # Ho = 49 = 4 x 12 + 1: 60 rows of 12-row tiles < 64 rows of 16-row tiles; input gradient 20 channels on 53 x 37: 12-row too
    Case("w5-12r-nt2", mf("5,12,16,2,3,false"), mf("5,12,16,2,3,false"), (8, 12), 32, 5, "reflect", (49, 33), (8, 0, 0)),
    Case("w5-24r-nt4", mf("5,24,16,4,6,false"), NT1_5, (16,), 64, 5, "replicate", (47, 15), (16, 0, 0)),
    Case("w5-24r-nt4-full", mf("5,24,16,4,6,false"), NT1_5, (11,), 64, 5, "zeros", (48, 33)),
    Case("w5-12r-nt4", mf("5,12,16,4,6,false,2x2"), NT1_5, (11,), 64, 5, "zeros", (49, 17), (16, 0, 0)),
    # sym_v and sym_hv in a 16-bit type: U = 64 - 4 - 2 - 6 = 52 unique filters; 8 input channels = half a K-chunk
    Case("w5-16r-nt4-vhv", mf("5,16,16,4,8,false,2x2"), mf("5,16,32,1,8,false"), (8,), 64, 5, "reflect", (95, 18), (8, 4, 8)),
    # ---- wide-tile, k = 3
    Case("w3-nt2-tile+1", mf("3,16,16,2,4,false"), mf("3,16,16,2,4,false"), (16, 8), 32, 3, "reflect", (17, 17), (8, 0, 0)),
    Case("w3-nt4-2tile-1", mf("3,16,16,4,8,false,2x2"), NT1_3, (11,), 64, 3, "zeros", (31, 31), (16, 0, 0)),
    Case("w3-nt2-small", mf("3,16,16,2,4,false"), NT1_3, (48,), 20, 3, "replicate", (5, 7), (4, 0, 0)),
    # ---- wide-tile with one N-tile and f32 output (16 x 32 tiles; 17 x 33 and 31 x 63 outputs): a head with full padding
    # (pad = k - 1) narrower than 140 columns.  k = 3:
    # the ConvAE curl head (engine.convae_graph, pad 2); k = 5: a stand-alone SymmetricConv2d(kernel 5, padding 4, c_out <= 16)
    Case("w3-nt1-f32out", mf("3,16,32,1,8,true"), NT1_3, (16,), 4, 3, "replicate", (15, 31), pad=2, out_f32=1),
    Case("w5-nt1-f32out", mf("5,16,32,1,8,true"), NT1_5, (11,), 4, 5, "reflect", (27, 59), pad=4, out_f32=1),
    # ---- row reuse, forward with one / three output tiles at a narrow width (input gradients: one N-tile wide-tile kernel)
    Case("rr5-1tile-w63", rr("5"), NT1_5, (16,), 16, 5, "reflect", (17, 63), (4, 0, 0)),
    Case("rr5-3tiles-2tile-1", rr("5"), NT1_5, (11,), 48, 5, "replicate", (31, 127), (12, 0, 0)),
    Case("rr5-small", rr("5"), NT1_5, (48,), 4, 5, "zeros", (5, 9)),
    Case("rr5-min-reflect", rr("5"), NT1_5, (16,), 16, 5, "reflect", (3, 3), (4, 0, 0)),
    # two output tiles at Wo >= 100; input gradient 20 channels on 22 x 133 (< 140): wide-tile, 8-row, split at 8
    Case("rr5-2tiles-w129", rr("5"), mf("5,8,16,2,2,false"), (8, 12), 20, 5, "reflect", (18, 129), (4, 0, 0)),
    # input gradient on the row-reuse kernel: padded width 136 + 4 = 140, without and (137 + 4 = 141) with c_out_split
    Case("rr5-dgrad-w140", rr("5"), rr("5"), (16,), 32, 5, "replicate", (17, 136), (8, 0, 0)),
    Case("rr5-dgrad-split", rr("5"), rr("5"), (16, 8), 16, 5, "zeros", (20, 137), (4, 0, 0)),
    Case("rr3-1tile-w65", rr("3"), NT1_3, (48,), 16, 3, "zeros", (17, 65), (4, 0, 0)),
    Case("rr3-3tiles-small", rr("3"), NT1_3, (16,), 48, 3, "reflect", (5, 63), (12, 0, 0)),
    Case("rr3-2tiles-dgrad-split", rr("3"), rr("3"), (16, 8), 32, 3, "replicate", (31, 138), (8, 0, 0)),
    Case("rr3-dgrad-w141", rr("3"), rr("3"), (11,), 20, 3, "reflect", (15, 139), (4, 0, 0)),
    Case("rr5-f32out", rr("5,f32out"), NT1_5, (16,), 4, 5, "reflect", (17, 65), out_f32=1),
    Case("rr3-f32out", rr("3,f32out"), NT1_3, (8,), 4, 3, "zeros", (9, 129), out_f32=1),
    # ---- persistent loop.  Row reuse (rr_launch): 256 / groups work-groups per output-tile column, groups = ceil(48 / 16) = 3
    # -> 85; tiles = ceil(33 / 16) x ceil(577 / 64) = 3 x 10 = 30, N = 3: 90 items > 85, the first five work-groups walk two
    Case("rr3-persistent", rr("3"), rr("3"), (8,), 48, 3, "reflect", (33, 577), (12, 0, 0), n=3),
    # Wide-tile (mc_conv2d_bf16): 4096 / groups, 192 channels = 12 N-tiles in groups of 4 -> groups = 3 -> 1365 (12 output tiles
    # never take row reuse); 8-row tiles at Ho = 33 <= 40: tiles = ceil(33 / 8) x ceil(1457 / 16) = 5 x 92 = 460, N = 3: 1380 > 1365
    Case("w5-persistent", mf("5,8,16,4,4,false,2x2"), rr("5"), (8,), 192, 5, "replicate", (33, 1457), (48, 0, 0), n=3),
    # ---- f32 direct kernels (16 x 16 tiles)
    Case("f32-k5-tile+1", direct(5), direct(5), (11,), 20, 5, "reflect", (17, 17), (4, 0, 0), f32=True),
    Case("f32-k5-small", direct(5), direct(5), (16,), 16, 5, "replicate", (7, 9), (4, 0, 0), f32=True),
    Case("f32-k5-min-reflect", direct(5), direct(5), (16, 8), 4, 5, "reflect", (3, 3), f32=True),
    Case("f32-k3-2tile-1", direct(3), direct(3), (8, 12), 20, 3, "zeros", (31, 31), (4, 2, 4), f32=True),
    Case("f32-k3-small", direct(3), direct(3), (48,), 16, 3, "replicate", (5, 7), (4, 0, 0), f32=True),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)

# the instantiations the table must reach, forward and input-gradient descriptors together
KERNELS = {
    direct(3), direct(5),
    mf("5,8,16,2,2,false"), mf("5,8,16,4,4,false,2x2"), mf("5,16,16,2,4,false"), mf("5,12,16,2,3,false"),
    mf("5,24,16,4,6,false"), mf("5,12,16,4,6,false,2x2"), mf("5,16,16,4,8,false,2x2"),
    mf("3,16,16,2,4,false"), mf("3,16,16,4,8,false,2x2"),
    NT1_5, NT1_3, mf("5,16,32,1,8,true"), mf("3,16,32,1,8,true"),
    rr("3"), rr("5"), rr("3,f32out"), rr("5,f32out"),
}

# (case id, precision) of every run: a 16-bit case runs as MC_BF16 and as MC_MIX16 (the H16 forward kernels on
# mfma_f32_16x16x32_f16, the XH filter gradient: x in f16, dy in bf16)
RUNS = [(c.id, dt) for c in CASES for dt in (("f32",) if c.f32 else ("bf16", "mix16"))]
RUN_IDS = [f"{i}-{dt}" for i, dt in RUNS]
MC = {"f32": L.MC_F32, "bf16": L.MC_BF16, "mix16": L.MC_MIX16}

# element type and unit roundoff by role: forward tensors (x, y, forward bank) / gradient tensors (dy, dx, input-gradient bank)
FWD_T = {"f32": torch.float32, "bf16": torch.bfloat16, "mix16": torch.float16}
GRAD_T = {"f32": torch.float32, "bf16": torch.bfloat16, "mix16": torch.bfloat16}
UNIT = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
F16_SPACING = 2.0 ** -24              # subnormal spacing of f16: the absolute term of an f16 store


def tile_of(kernel):
    """(rows, columns) of the output tile of a kernel instantiation."""
    if kernel.startswith("k_conv_mfma_bf16<"):
        a = kernel[len("k_conv_mfma_bf16<"):].split(",")
        return int(a[1]), int(a[2])
    return (16, 64) if kernel.startswith("k_conv_rr_bf16") else (16, 16)


def pad_of(c):
    return c.k // 2 if c.pad < 0 else c.pad


def out_hw(c):
    p = pad_of(c)
    return c.hw[0] + 2 * p - c.k + 1, c.hw[1] + 2 * p - c.k + 1


def descs(c, dt):
    """(forward descriptor, input-gradient descriptor), as engine._conv_descs builds them: the input gradient is the same
    kernel on the padded domain (zero padding k - 1), MC_BF16 for an MC_MIX16 layer, split at c_in0 for two sources."""
    mc = MC[dt]
    mcg = L.MC_BF16 if mc == L.MC_MIX16 else mc
    ci0, ci1 = c.ci[0], (c.ci[1] if len(c.ci) > 1 else 0)
    ho, wo = out_hw(c)
    d = L.ConvDesc(c.n, c.hw[0], c.hw[1], ci0, ci1, c.co, c.k, pad_of(c), L.PAD_MODES[c.mode], mc, c.sym[0], 0, c.out_f32,
                   c.sym[1], c.sym[2])
    dd = L.ConvDesc(c.n, ho, wo, c.co, 0, ci0 + ci1, c.k, c.k - 1, 0, mcg, 0, ci0 if ci1 else 0, 0, 0, 0)
    return d, dd


def kernel_name(d):
    return L.load().mc_conv_kernel_name(C.byref(d)).decode()


# ---- operands -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(x, w_unique, bias, cotangent) in f32, as they are handed to the library."""
    c = CASE_BY_ID[case_id]
    g = torch.Generator().manual_seed(4000 + CASES.index(c))
    cin = sum(c.ci)
    u = c.co - c.sym[0] // 2 - c.sym[1] // 2 - 3 * (c.sym[2] // 4)
    x = torch.randn((c.n, cin, *c.hw), generator=g)
    wu = torch.randn((u, cin, c.k, c.k), generator=g) / (cin * c.k * c.k) ** 0.5
    b = 0.1 * torch.randn((c.co,), generator=g)
    ct = torch.randn((c.n, c.co, *out_hw(c)), generator=g)
    return x, wu, b, ct


def rnd(t, *types):
    """t rounded through the given storage types in turn (round to nearest even, as the pack kernels round), in f64."""
    for ty in types:
        t = t.to(ty)
    return t.double()


def sym_dict(c):
    return {"h": c.sym[0], "v": c.sym[1], "hv": c.sym[2]}


def expand_unflipped(wu, c):
    """The mutant bank: the mirrored copies in the reference's order, left unflipped."""
    nh, nv, nq = c.sym[0] // 2, c.sym[1] // 2, c.sym[2] // 4
    blk = wu[nh + nv:nh + nv + nq]
    return torch.cat([wu, wu[:nh], wu[nh:nh + nv], blk, blk, blk], 0)


# ---- the tolerance ------------------------------------------------------------------------------------------------------
def tolerance(ref, S, K, u, f=0.0):
    """Per element tol = E + u (|ref| + E) + f, E = (K + 1) 2^-24 S: f32 accumulation of K exact products (+ bias) in any
    order, then one rounding to the stored type (unit roundoff u; f = the f16 subnormal spacing)."""
    E = (K + 1) * 2.0 ** -24 * S
    return E + u * (ref.abs() + E) + f


def compare(got, ref, tol):
    """(worst err / tol, mask of failing elements).  A NaN fails."""
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    ratio = torch.nan_to_num(err / tol.clamp_min(1e-300), nan=float("inf"))
    return (float(ratio.max()) if ratio.numel() else 0.0), bad


def forward_eval(c, x64, wfull64, b64, mode=None):
    p = pad_of(c)
    return O.conv2d_same(x64, wfull64, b64, mode or c.mode, padding=(p, p))


class FwdRef(NamedTuple):
    y: torch.Tensor            # f64, unrounded
    tol: torch.Tensor
    E: torch.Tensor            # the accumulation part of tol: bound on |f32 accumulator - y|
    store: torch.dtype         # element type of the stored output


@functools.lru_cache(maxsize=None)
def forward_ref(case_id, dt):
    c = CASE_BY_ID[case_id]
    x, wu, b, _ = inputs(case_id)
    ft = FWD_T[dt]
    x64, w64, b64 = rnd(x, ft), rnd(wu, ft), b.double()
    y = forward_eval(c, x64, O.expand_symmetric_weight(w64, sym_dict(c)), b64)
    S = forward_eval(c, x64.abs(), O.expand_symmetric_weight(w64.abs(), sym_dict(c)), b64.abs())
    K = c.k * c.k * sum(c.ci)
    store = torch.float32 if c.out_f32 else ft
    tol = tolerance(y, S, K, UNIT[store], F16_SPACING if store == torch.float16 else 0.0)
    return FwdRef(y, tol, (K + 1) * 2.0 ** -24 * S, store)


def stats_ref(case_id, dt):
    """Per (n, c): (sum y, sum y^2) of the unrounded reference and their bounds.  The kernel sums its f32 accumulators a_i,
    |a_i - y_i| <= E_i, over the M = Ho Wo pixels in f32 in some order (the test adds the tile partials in f64):
      |sum a - sum y|     <= sum E_i + (M + 1) 2^-24 sum (|y_i| + E_i)
      |sum a^2 - sum y^2| <= sum (2 |y_i| E_i + E_i^2) + (M + 2) 2^-24 sum (|y_i| + E_i)^2   (one more rounding: the square)"""
    r = forward_ref(case_id, dt)
    M = r.y.shape[2] * r.y.shape[3]
    a = r.y.abs() + r.E
    ref = torch.stack([r.y.sum((2, 3)), (r.y * r.y).sum((2, 3))], -1)
    t1 = r.E.sum((2, 3)) + (M + 1) * 2.0 ** -24 * a.sum((2, 3))
    t2 = (2 * r.y.abs() * r.E + r.E * r.E).sum((2, 3)) + (M + 2) * 2.0 ** -24 * (a * a).sum((2, 3))
    return ref, torch.stack([t1, t2], -1)


@functools.lru_cache(maxsize=None)
def dgrad_ref(case_id, dt):
    """Gradient w.r.t. the PADDED input: conv_transpose2d of the cotangent with the full bank, both in the gradient type."""
    c = CASE_BY_ID[case_id]
    _, wu, _, ct = inputs(case_id)
    gt = GRAD_T[dt]
    ct64, w64 = rnd(ct, gt), O.expand_symmetric_weight(rnd(wu, gt), sym_dict(c))
    ref = F.conv_transpose2d(ct64, w64)
    S = F.conv_transpose2d(ct64.abs(), w64.abs())
    return ref, tolerance(ref, S, c.k * c.k * c.co, UNIT[gt])


WGRAD_PREFILL = 0.25          # mc_conv2d_wgrad_finalize accumulates: dw / dbias start at this value (exact in f32)


@functools.lru_cache(maxsize=None)
def wgrad_ref(case_id, dt):
    """(dw_unique, tol, dbias, tol) INCLUDING the prefill.  x is read in the forward type (MC_MIX16: f16, converted to bf16
    while the tile is staged), dy in the gradient type; f32 sums of K = N Ho Wo x (copies folded onto the unique filter)
    products, plus the prefill as one more addend (so it enters S like a bias)."""
    c = CASE_BY_ID[case_id]
    x, wu, b, ct = inputs(case_id)
    xt = (torch.float16, torch.bfloat16) if dt == "mix16" else (FWD_T[dt],)
    x64, ct64 = rnd(x, *xt), rnd(ct, GRAD_T[dt])

    def grads(xx, cc):
        w = torch.zeros(wu.shape, dtype=torch.float64, requires_grad=True)     # (the gradient is independent of w and b)
        bb = torch.zeros(b.shape, dtype=torch.float64, requires_grad=True)
        (forward_eval(c, xx, O.expand_symmetric_weight(w, sym_dict(c)), bb) * cc).sum().backward()
        return w.grad, bb.grad
    dw, db = grads(x64, ct64)
    sw, sb = grads(x64.abs(), ct64.abs())
    ho, wo = out_hw(c)
    px = c.n * ho * wo
    nh, nv, nq = c.sym[0] // 2, c.sym[1] // 2, c.sym[2] // 4
    copies = torch.ones(wu.shape[0], dtype=torch.float64)
    copies[:nh + nv] = 2
    copies[nh + nv:nh + nv + nq] = 4
    dw, db = dw + WGRAD_PREFILL, db + WGRAD_PREFILL
    tw = tolerance(dw, sw + WGRAD_PREFILL, (px * copies).view(-1, 1, 1, 1), 0.0)
    tb = tolerance(db, sb + WGRAD_PREFILL, px, 0.0)
    return dw, tw, db, tb

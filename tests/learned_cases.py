"""Case table, operands, f64 references and the derived bounds of tests/test_hip_learned_kernels.py: the learned-padding frame
kernels of csrc/conv_learned.hip (bank packing, frame forward, frame input gradient, frame filter gradient and its reduce).

The reference is oracle.ref_cpu.boundary_learned_conv in f64 with autograd, on operands rounded to what each kernel reads; the
absolute-value companion S of every reference is the same expression on |x|, |w|, |bias|, |ct|; the bound per element is
conv_variants.tolerance with K counted from the geometry (engine.learned_regions).  The frame's share of a gradient is taken
from the whole operator with the cotangent zeroed on the interior rectangle, the main bank's share with it zeroed on the frame.
Nothing here touches a device."""
import ctypes as C
import functools
from types import SimpleNamespace
from typing import NamedTuple, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_variants as V
from oracle import ref_cpu as O
from pbml_mantle_convection_amd import _lib as L
from pbml_mantle_convection_amd.engine import learned_regions

ALL = ("f32", "bf16", "mix16")


class Case(NamedTuple):
    id: str
    ci: int
    co: int
    k: int
    symm: bool
    bc_x: int
    bc_y: int
    h: int
    w: int
    n: int
    dts: Tuple[str, ...] = ALL
    wgrad_only: bool = False          # filter gradient only; the f64 oracle is evaluated on the banks' strips


CASES = [
    # CT = 3, IT = 2, both last tiles half filled; sym_h = 10: the mirrored copies co 35..39 (tile 2) fold onto u 0..4 (tile 0)
    Case("tiles", 24, 40, 5, True, 1, 1, 9, 21, 3),
    # the roles of the two sides swapped (CT = 2, IT = 3); J = 45 padded to 48; bc_x != bc_y
    Case("tiles-k3", 40, 24, 3, True, 2, 1, 5, 9, 2),
    # the U-Net's first layer (bc_x = 4): h = 2 pad_y, the row bands exactly meet; w = 2 pad_x + 1
    Case("first-layer", 10, 32, 5, True, 4, 1, 12, 19, 3),
    # h = pad_y, w = pad_x: every source rectangle is the whole input, every pixel is read by all eight banks
    Case("minimal-k5", 8, 16, 5, True, 1, 1, 6, 6, 2),
    Case("minimal-k3", 16, 8, 3, False, 1, 1, 3, 3, 3),
    # top / bottom: rh = 3, rw = 11 -> 33 = 2 * 16 + 1 output pixels, 99 visits (odd); unaligned channel counts.  With bc_x = 1
    # the bands hold 14 * 15 + 12 (h - 14) input pixels for h >= 14 and 15 h below: never 1 mod 16 (even, or h = 15 >= 14) ...
    Case("group-seam", 7, 20, 5, False, 1, 2, 15, 15, 3),
    # ... so the band seam has a case of its own: bc_x = 3 is the smallest that makes the column bands 15 = w wide, 15 * 15 = 225
    Case("band-seam", 7, 20, 5, False, 3, 2, 15, 15, 3),
    # top / bottom: 2 * 2 * 146 = 584 visits -> 10 slices in f32, 5 in 16-bit; h < 2 pad_y: the row bands overlap
    Case("long-row", 16, 16, 5, True, 1, 1, 8, 150, 2),
    # slab 1.6 MB -> smax = 40: the slice length leaves its floor once the visits pass 40 * 64 (f32) / 40 * 128 (16-bit).
    # visits = n (4 (h + w) - 16); at n = 4 and h = pad_y, the smallest height, these are the smallest widths at which the longer
    # slices save a slab (w = 165: 2672 visits, SL = 67; w = 325: 5232 visits, SL = 131)
    Case("slice-length-f32", 128, 128, 5, True, 1, 1, 6, 165, 4, ("f32",), True),
    Case("slice-length-16", 128, 128, 5, True, 1, 1, 6, 325, 4, ("bf16", "mix16"), True),
]
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)
FULL_CASES = [c for c in CASES if not c.wgrad_only]

RUNS = [(c.id, dt) for c in FULL_CASES for dt in c.dts]
RUN_IDS = [f"{i}-{dt}" for i, dt in RUNS]
WGRAD_RUNS = [(c.id, dt) for c in CASES for dt in c.dts]
WGRAD_RUN_IDS = [f"{i}-{dt}" for i, dt in WGRAD_RUNS]

FRAME_BANKS = L.LEARNED_FRAME_BANKS           # the order of the bank arrays of the mc_learned_* entry points
DW_PREFILL = tuple(0.25 * (b + 1) for b in range(8))     # dW of bank b starts at this value, dbias at DB_PREFILL (exact in f32)
DB_PREFILL = 0.5


# ---- geometry -----------------------------------------------------------------------------------------------------------
def sym_dict(c):
    return O.symmetry_counts(c.co) if c.symm else {"h": 0, "v": 0, "hv": 0}


@functools.lru_cache(maxsize=None)
def geometry(cid):
    """The numbers conv_learned.hip's l_geom derives, from engine.learned_regions.  regs: frame bank -> (sy, sx, sh, sw, dy,
    dx, rh, rw) = source rectangle, destination origin, destination rectangle."""
    c = CASE_BY_ID[cid]
    fy, fx, ho, wo, regs = learned_regions(c.h, c.w, c.k, c.bc_x, c.bc_y)
    pad_x, pad_y = fx + c.k - 1, fy + c.k - 1
    g = SimpleNamespace(fy=fy, fx=fx, ho=ho, wo=wo, pad_x=pad_x, pad_y=pad_y, mh=c.h - c.k + 1, mw=c.w - c.k + 1, kk=c.k * c.k)
    g.regs = {b: (*regs[b], regs[b][2] - c.k + 1, regs[b][3] - c.k + 1) for b in FRAME_BANKS}
    g.main = regs["conv"]
    g.cbin, g.cbout, g.ct, g.it = (c.ci + 7) // 8, (c.co + 7) // 8, (c.co + 15) // 16, (c.ci + 15) // 16
    g.j, g.jd = g.cbin * g.kk, g.cbout * g.kk
    g.jp, g.jdp = (g.j + 15) // 16 * 16, (g.jd + 15) // 16 * 16
    g.sym_h = sym_dict(c)["h"]
    g.nh = g.sym_h // 2
    g.u = c.co - g.nh
    g.nrb, g.ncb = min(c.h, 2 * pad_y), min(c.w, 2 * pad_x)
    g.band_pix = g.nrb * c.w + (c.h - g.nrb) * g.ncb
    g.visits = {b: c.n * r[6] * r[7] for b, r in g.regs.items()}
    frame = torch.ones((ho, wo), dtype=torch.bool)
    frame[fy:fy + g.mh, fx:fx + g.mw] = False
    g.frame = frame
    readers = torch.zeros((c.h, c.w), dtype=torch.int64)          # frame banks whose source rectangle holds the input pixel
    for sy, sx, sh, sw, *_ in g.regs.values():
        readers[sy:sy + sh, sx:sx + sw] += 1
    g.readers = readers
    return g


def desc(c, dt):
    return L.LearnedDesc(c.n, c.h, c.w, c.ci, c.co, c.k, c.bc_x, c.bc_y, V.MC[dt], geometry(c.id).sym_h)


def slab_bytes(c):
    g = geometry(c.id)
    return 4 * (g.kk * g.ct * g.it * 256 + g.ct * 16)


def slmin(dt):
    return 64 if dt == "f32" else 128


def slabs(c, dt):
    """Partial slabs of the filter gradient, from the size query."""
    nbytes = L.load().mc_learned_wgrad_workspace_bytes(C.byref(desc(c, dt)))
    assert nbytes > 0 and nbytes % slab_bytes(c) == 0
    return nbytes // slab_bytes(c)


# ---- operands -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(x, {bank: unique filters}, bias, cotangent) in f32, as they are handed to the library (the nine banks, the main one
    included; none for a filter-gradient-only case)."""
    c = CASE_BY_ID[cid]
    g = geometry(cid)
    gen = torch.Generator().manual_seed(7000 + CASES.index(c))
    x = torch.randn((c.n, c.ci, c.h, c.w), generator=gen)
    ws = {}
    if not c.wgrad_only:
        ws = {b: torch.randn((g.u, c.ci, c.k, c.k), generator=gen) / (c.ci * g.kk) ** 0.5 for b in O.LEARNED_BANKS}
    b = 0.5 * torch.randn((c.co,), generator=gen)
    ct = torch.randn((c.n, c.co, g.ho, g.wo), generator=gen)
    return x, ws, b, ct


def x_types(dt):
    """What the filter gradient reads of x: MC_MIX16 converts the f16 activation to bf16 on load."""
    return (torch.float16, torch.bfloat16) if dt == "mix16" else (V.FWD_T[dt],)


def state_dict(c, ws, bias):
    sd = {b + ".weight": w for b, w in ws.items()}
    sd["learnable_bias"] = bias.reshape(1, c.co, 1, 1)
    return sd


def operator(c, x, ws, bias):
    return O.boundary_learned_conv(state_dict(c, ws, bias), "", x, c.k, c.symm, c.bc_x, c.bc_y)


def split_ct(c, ct):
    """(the cotangent on the frame, on the interior rectangle): zero elsewhere."""
    f = geometry(c.id).frame.to(ct.dtype)
    return ct * f, ct * (1 - f)


# ---- evaluations in the operands' own type (f64 for the references, f32 for the host check of the bounds) -----------------
def dx_eval(c, ws, ct):
    """(main bank's input gradient, the frame's): autograd of the whole operator, the cotangent split."""
    x = torch.zeros((c.n, c.ci, c.h, c.w), dtype=ct.dtype, requires_grad=True)     # (the operator is linear in x)
    y = operator(c, x, ws, torch.zeros(c.co, dtype=ct.dtype))
    ctf, cti = split_ct(c, ct)
    main, = torch.autograd.grad((y * cti).sum(), x, retain_graph=True)
    frame, = torch.autograd.grad((y * ctf).sum(), x)
    return main, frame


def wg_eval(c, x, ct):
    """({frame bank: dW of the unique filters}, dbias of the frame), without the prefill."""
    g = geometry(c.id)
    ctf, _ = split_ct(c, ct)
    if c.wgrad_only:
        out = {}
        for b, (sy, sx, sh, sw, dy, dx, rh, rw) in g.regs.items():
            w = torch.zeros((g.u, c.ci, c.k, c.k), dtype=x.dtype, requires_grad=True)
            y = F.conv2d(x[:, :, sy:sy + sh, sx:sx + sw], O.expand_symmetric_weight(w, sym_dict(c)) if c.symm else w)
            out[b], = torch.autograd.grad((y * ct[:, :, dy:dy + rh, dx:dx + rw]).sum(), w)
        return out, ctf.sum((0, 2, 3))
    ws = {b: torch.zeros((g.u, c.ci, c.k, c.k), dtype=x.dtype, requires_grad=b != "conv") for b in O.LEARNED_BANKS}
    bias = torch.zeros(c.co, dtype=x.dtype, requires_grad=True)          # (the gradients do not depend on w and bias)
    (operator(c, x, ws, bias) * ctf).sum().backward()
    return {b: ws[b].grad for b in FRAME_BANKS}, bias.grad


# ---- references and bounds ----------------------------------------------------------------------------------------------
class FwdRef(NamedTuple):
    y: torch.Tensor            # f64, the whole output; compared on the frame
    tol: torch.Tensor
    store: torch.dtype


@functools.lru_cache(maxsize=None)
def forward_ref(cid, dt, with_bias=True):
    c = CASE_BY_ID[cid]
    x, ws, b, _ = inputs(cid)
    ft = V.FWD_T[dt]
    x64, w64 = V.rnd(x, ft), {n: V.rnd(w, ft) for n, w in ws.items()}
    b64 = b.double() if with_bias else torch.zeros(c.co, dtype=torch.float64)
    y = operator(c, x64, w64, b64)
    S = operator(c, x64.abs(), {n: w.abs() for n, w in w64.items()}, b64.abs())
    tol = V.tolerance(y, S, c.k * c.k * c.ci, V.UNIT[ft], V.F16_SPACING if ft == torch.float16 else 0.0)
    return FwdRef(y, tol, ft)


class DxRef(NamedTuple):
    before: torch.Tensor       # what dX holds before the launch: the main bank's gradient in the gradient type
    dx: torch.Tensor           # before + the frame's gradient, f64
    tol: torch.Tensor
    store: torch.dtype


def dgrad_k(c):
    """K per input pixel [h][w]: k k c_out products per frame bank that reads the pixel."""
    return c.k * c.k * c.co * geometry(c.id).readers


@functools.lru_cache(maxsize=None)
def dgrad_ref(cid, dt):
    c = CASE_BY_ID[cid]
    _, ws, _, ct = inputs(cid)
    gt = V.GRAD_T[dt]
    ct64, w64 = V.rnd(ct, gt), {n: V.rnd(w, gt) for n, w in ws.items()}
    main, frame = dx_eval(c, w64, ct64)
    before = V.rnd(main, gt)
    _, sframe = dx_eval(c, {n: w.abs() for n, w in w64.items()}, ct64.abs())
    ref = before + frame
    tol = V.tolerance(ref, before.abs() + sframe, dgrad_k(c).double(), V.UNIT[gt])
    return DxRef(before, ref, tol, gt)


class WgRef(NamedTuple):
    dw: dict                   # frame bank -> (dW of the unique filters INCLUDING the prefill, tol)
    db: torch.Tensor           # INCLUDING the prefill
    db_tol: torch.Tensor


def wgrad_k(c, bank):
    """K per unique filter [U]: the bank's visits, twice for a filter with an x-mirrored copy."""
    g = geometry(c.id)
    k = torch.full((g.u,), float(g.visits[bank]), dtype=torch.float64)
    k[:g.nh] *= 2
    return k


def wgrad_operands(cid, dt, xt=None):
    c = CASE_BY_ID[cid]
    x, _, _, ct = inputs(cid)
    return c, V.rnd(x, *(xt or x_types(dt))), V.rnd(ct, V.GRAD_T[dt])


@functools.lru_cache(maxsize=None)
def wgrad_ref(cid, dt):
    c, x64, ct64 = wgrad_operands(cid, dt)
    g = geometry(cid)
    dw, db = wg_eval(c, x64, ct64)
    sw, sb = wg_eval(c, x64.abs(), ct64.abs())
    out = {}
    for i, b in enumerate(FRAME_BANKS):
        ref = dw[b] + DW_PREFILL[i]
        out[b] = (ref, V.tolerance(ref, sw[b] + DW_PREFILL[i], wgrad_k(c, b).view(-1, 1, 1, 1), 0.0))
    db = db + DB_PREFILL
    return WgRef(out, db, V.tolerance(db, sb + DB_PREFILL, c.n * (g.ho * g.wo - g.mh * g.mw), 0.0))


# ---- the operator restated on explicit rectangles and full banks: the mutants' workbench -----------------------------------
def full_banks(c, ws, unflipped=False):
    if not c.symm:
        return dict(ws)
    s = sym_dict(c)
    return {b: (V.expand_unflipped(w, SimpleNamespace(sym=(s["h"], 0, 0))) if unflipped else O.expand_symmetric_weight(w, s))
            for b, w in ws.items()}


def restated(c, x, wfull, bias, regs=None):
    """Nine valid convolutions placed by rectangle.  regs: bank -> (sy, sx, sh, sw, dy, dx, ...), the main bank under 'conv'."""
    g = geometry(c.id)
    regs = dict(g.regs, conv=g.main) if regs is None else regs
    y = torch.zeros((c.n, c.co, g.ho, g.wo), dtype=x.dtype)
    for b, (sy, sx, sh, sw, dy, dx, *_) in regs.items():
        y[:, :, dy:dy + sh - c.k + 1, dx:dx + sw - c.k + 1] = F.conv2d(x[:, :, sy:sy + sh, sx:sx + sw], wfull[b])
    return y + bias.view(1, -1, 1, 1)


def visit_term(c, bank, x, ct, n, ty, tx):
    """One visit's contribution to the gradient of the bank's FULL filters [co][ci][k][k]."""
    sy, sx, _, _, dy, dx, _, _ = geometry(c.id).regs[bank]
    return ct[n, :, dy + ty, dx + tx].view(-1, 1, 1, 1) * x[n, :, sy + ty:sy + ty + c.k, sx + tx:sx + tx + c.k].unsqueeze(0)


def fold(c, gfull):
    """Gradient of the full bank -> gradient of the unique filters (the mirrored copies' flipped in x and added)."""
    g = geometry(c.id)
    out = gfull[:g.u].clone()
    out[:g.nh] += gfull[g.u:].flip(3)
    return out


# ---- the bank layout, restated from the header comment of conv_learned.hip ------------------------------------------------
def bank_layout(c, dt):
    """(forward bank, input-gradient bank) as typed CPU tensors.
    forward:        [bank 8][co tile][pair j = cb * k*k + tap, padded to 16][co 16][ci 8]
    input gradient: [bank 8][ci tile][pair j = cbo * k*k + tap, padded to 16][ci 16][co 8]
    mirrored filters flipped in x; padding pairs, channels and rows zero; forward f16 for mix16, input gradient bf16."""
    g = geometry(c.id)
    ws = inputs(c.id)[1]
    full = np.zeros((8, g.ct * 16, g.it * 16, g.kk), dtype=np.float32)
    for i, b in enumerate(FRAME_BANKS):
        wu = ws[b].numpy()
        w = np.concatenate([wu, wu[:g.nh, :, :, ::-1]], 0) if c.symm else wu
        full[i, :c.co, :c.ci] = w.reshape(c.co, c.ci, g.kk)
    fwd = np.zeros((8, g.ct, g.jp, 16, 8), dtype=np.float32)
    src = full[:, :, :g.cbin * 8].reshape(8, g.ct, 16, g.cbin, 8, g.kk)             # [b][tile][row][cb][e][tap]
    fwd[:, :, :g.j] = src.transpose(0, 1, 3, 5, 2, 4).reshape(8, g.ct, g.j, 16, 8)
    dg = np.zeros((8, g.it, g.jdp, 16, 8), dtype=np.float32)
    src = full[:, :g.cbout * 8].reshape(8, g.cbout, 8, g.it, 16, g.kk)              # [b][cbo][e][tile][row][tap]
    dg[:, :, :g.jd] = src.transpose(0, 3, 1, 5, 4, 2).reshape(8, g.it, g.jd, 16, 8)
    return torch.from_numpy(fwd).to(V.FWD_T[dt]), torch.from_numpy(dg).to(V.GRAD_T[dt])

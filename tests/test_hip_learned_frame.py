"""GPU tests of the learned-padding frame kernels (csrc/conv_learned.hip) through the raw C ABI, against
oracle.ref_cpu.boundary_learned_conv in float64 with autograd gradients; whole-layer parity and the launch budget through
the engine and the stand-alone module.

Tolerances are the project's own for this layer: fp32 the three bounds of test_boundary_learned_conv_vs_golden; 16-bit
stored results 8e-3 (bf16) / 1e-3 (f16) of |ref|max, 16-bit filter and bias gradients 2e-2 of |ref|max (test_hip_parity.py).
For the 16-bit modes the oracle is fed the inputs already rounded to the storage types."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 2
# name: (c_i, c_o, k, symm, bc_x, bc_y, h, w)
CASES = {
    "unet_first_20x141": (10, 16, 5, True, 4, 1, 20, 141),    # crosses a column tile; the bands do not cover the input
    "deepest_8x31": (16, 16, 5, True, 1, 1, 8, 31),           # top and bottom bands overlap
    "tiny_6x7": (6, 6, 5, False, 1, 1, 6, 7),                 # every strip is the whole input; unaligned channels
    "fluidnet_head_16x17": (7, 16, 5, True, 2, 2, 16, 17),
    "k3_head_4x5": (16, 4, 3, True, 1, 1, 4, 5),
}
# precision: (MC dtype, forward tensor type, gradient tensor type)
PREC = {"fp32": (0, torch.float32, torch.float32), "bf16": (1, torch.bfloat16, torch.bfloat16),
        "mixed": (2, torch.float16, torch.bfloat16)}
SENTINEL = 7.25


def _L():
    from pbml_mantle_convection_amd import _lib as L
    L.load()
    return L


def to_cb8(t, dtype):
    n, c, h, w = t.shape
    c8 = (c + 7) // 8
    p = torch.zeros((n, c8 * 8, h, w), dtype=torch.float64)
    p[:, :c] = t
    return p.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dtype).to(DEV)


def from_cb8(buf, c):
    n, c8, h, w, _ = buf.shape
    return buf.detach().cpu().double().permute(0, 1, 4, 2, 3).reshape(n, c8 * 8, h, w)[:, :c]


def assert_close(a, b, atol, rtol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    print(f"{what}: max err {err.max():.3e}, |ref|max {np.abs(b).max():.3e}, atol {atol:.3e}, rtol {rtol:.1e}")
    assert (err <= atol + rtol * np.abs(b)).all(), f"{what}: max err {err.max():.3e} (tol {atol:.3e} + {rtol} |ref|)"


def tol(kind, precision, ref, stored=None):
    """(atol, rtol).  kind: y | dx | param.  stored: the 16-bit type the compared tensor is stored in."""
    m = float(np.abs(np.asarray(ref)).max())
    if precision == "fp32":
        a, r = {"y": (2e-5, 1e-4), "dx": (5e-5, 1e-3), "param": (2e-4, 2e-3)}[kind]
        return a * max(1.0, m), r
    if kind == "param":
        return 2e-2 * m, 0.0
    return (8e-3 if stored == torch.bfloat16 else 1e-3) * m, 0.0


@functools.lru_cache(maxsize=None)
def oracle(case, lowp):
    """Seeded inputs and the float64 reference of one case.  lowp = None (fp32) or the forward storage type: x is rounded to
    it, the filters, the bias-free output gradient `ct` to bf16 (exact in f16 as well), so the reference sees what the
    kernels read."""
    c_i, c_o, k, symm, bc_x, bc_y, h, w = CASES[case]
    gen = torch.Generator().manual_seed(1234 + sorted(CASES).index(case))
    sym = O.symmetry_counts(c_o) if symm else {"h": 0, "v": 0, "hv": 0}
    u = O.unique_filters(c_o, sym)

    def rnd(t, dt):
        return t.to(dt).double() if dt is not None else t.float().double()

    x = rnd(torch.randn((N, c_i, h, w), generator=gen), lowp)
    sd = {b + ".weight": rnd(0.1 * torch.randn((u, c_i, k, k), generator=gen), torch.bfloat16 if lowp else None)
          for b in O.LEARNED_BANKS}
    sd["learnable_bias"] = (0.5 * torch.randn((1, c_o, 1, 1), generator=gen)).float().double()
    for t in sd.values():
        t.requires_grad_(True)
    x.requires_grad_(True)
    y = O.boundary_learned_conv(sd, "", x, k, symm, bc_x, bc_y)
    ct = rnd(torch.randn(y.shape, generator=gen), torch.bfloat16 if lowp else None)
    (y * ct).sum().backward()
    pad_x = k + 1 + (bc_x - 1) if k == 5 else k + (bc_x - 1)
    pad_y = k + 1 + (bc_y - 1) if k == 5 else k + (bc_y - 1)
    fx, fy, mh, mw = pad_x - k + 1, pad_y - k + 1, h - k + 1, w - k + 1
    frame = torch.ones(y.shape[2:], dtype=torch.bool)
    frame[fy:fy + mh, fx:fx + mw] = False
    # the main bank alone: what dX holds before the frame launch, and the interior's share of the bias gradient
    xm = x.detach().clone().requires_grad_(True)
    wm = sd["conv.weight"].detach()
    ym = F.conv2d(xm, O.expand_symmetric_weight(wm, sym) if symm else wm)
    (ym * ct[:, :, fy:fy + mh, fx:fx + mw]).sum().backward()
    return dict(x=x.detach(), sd={n: t.detach() for n, t in sd.items()}, y=y.detach(), ct=ct, dx=x.grad, dx_main=xm.grad,
                grads={n: t.grad for n, t in sd.items()}, db_frame=(ct * frame).sum((0, 2, 3)), frame=frame,
                geo=(pad_x, pad_y, fx, fy, mh, mw), sym_h=sym["h"] if symm else 0)


class Frame:
    """Device state of one case in one precision: descriptor, packed banks, tensors; the three launches."""

    def __init__(self, case, precision):
        L = _L()
        self.L, self.case, self.precision = L, case, precision
        c_i, c_o, k, symm, bc_x, bc_y, h, w = CASES[case]
        self.mc, self.tx, self.tg = PREC[precision]
        self.o = o = oracle(case, None if precision == "fp32" else self.tx)
        self.c_i, self.c_o, self.h, self.w = c_i, c_o, h, w
        self.d = L.LearnedDesc(N, h, w, c_i, c_o, k, bc_x, bc_y, self.mc, o["sym_h"])
        assert L.call("mc_learned_validate", C.byref(self.d)) == 0
        self.st = L.stream()
        u8 = dict(dtype=torch.uint8, device=DEV)
        self.ws = [o["sd"][b + ".weight"].float().contiguous().to(DEV) for b in L.LEARNED_FRAME_BANKS]
        self.bias = o["sd"]["learnable_bias"].float().reshape(-1).contiguous().to(DEV)
        self.bank = torch.empty(L.call("mc_learned_bank_bytes", C.byref(self.d), 0), **u8)
        self.dbank = torch.empty(L.call("mc_learned_bank_bytes", C.byref(self.d), 1), **u8)
        self.work = torch.empty(L.call("mc_learned_wgrad_workspace_bytes", C.byref(self.d)), **u8)
        L.call("mc_learned_pack_banks_batched", C.byref(self.d), (C.c_void_p * 8)(*[L.ptr(t) for t in self.ws]),
               (C.c_void_p * 1)(L.ptr(self.bank)), (C.c_void_p * 1)(L.ptr(self.dbank)), 1, self.st)
        self.X = to_cb8(o["x"], self.tx)
        self.dYb = to_cb8(o["ct"], self.tg)

    def forward(self):
        L, o = self.L, self.o
        ho, wo = o["y"].shape[2:]
        Y = torch.full((N, (self.c_o + 7) // 8, ho, wo, 8), SENTINEL, dtype=self.tx, device=DEV)
        L.call("mc_learned_frame_fwd", C.byref(self.d), L.ptr(self.X), L.ptr(self.bank), L.ptr(self.bias), L.ptr(Y), self.st)
        return Y

    def dgrad(self):
        L = self.L
        dX = to_cb8(self.o["dx_main"], self.tg)
        before = dX.clone()
        L.call("mc_learned_frame_dgrad", C.byref(self.d), L.ptr(self.dYb), L.ptr(self.dbank), L.ptr(dX), self.st)
        return before, dX

    def wgrad(self):
        L = self.L
        dws = [torch.full_like(t, 0.5) for t in self.ws]
        db = torch.full((self.c_o,), 0.25, dtype=torch.float32, device=DEV)
        L.call("mc_learned_frame_wgrad", C.byref(self.d), L.ptr(self.X), L.ptr(self.dYb), L.ptr(self.work),
               (C.c_void_p * 8)(*[L.ptr(t) for t in dws]), L.ptr(db), self.st)
        return dws, db


@pytest.mark.parametrize("precision", list(PREC))
@pytest.mark.parametrize("case", list(CASES))
def test_frame_forward(case, precision):
    f = Frame(case, precision)
    o = f.o
    Y = f.forward()
    torch.cuda.synchronize()
    pad_x, pad_y, fx, fy, mh, mw = o["geo"]
    frame = o["frame"]
    got = from_cb8(Y, f.c_o)
    a, r = tol("y", precision, o["y"][:, :, frame], stored=f.tx)
    assert_close(got[:, :, frame], o["y"][:, :, frame], a, r, f"{case} {precision} y[frame]")
    # every element outside the frame is untouched (bit-equal to the sentinel), padded channels of the frame are zero
    inner = Y[:, :, fy:fy + mh, fx:fx + mw, :]
    assert torch.equal(inner, torch.full_like(inner, SENTINEL))
    if f.c_o % 8:
        tail = Y.detach().cpu().float().permute(0, 1, 4, 2, 3).reshape(N, -1, *Y.shape[2:4])[:, f.c_o:]
        assert (tail[:, :, frame] == 0).all(), "tail channels of the frame must be stored as zero"


@pytest.mark.parametrize("precision", list(PREC))
@pytest.mark.parametrize("case", list(CASES))
def test_frame_input_gradient(case, precision):
    f = Frame(case, precision)
    o = f.o
    before, dX = f.dgrad()
    torch.cuda.synchronize()
    a, r = tol("dx", precision, o["dx"], stored=f.tg)
    assert_close(from_cb8(dX, f.c_i), o["dx"], a, r, f"{case} {precision} dx")
    pad_x, pad_y = o["geo"][:2]
    if f.c_i % 8:
        assert (dX.cpu().float().permute(0, 1, 4, 2, 3).reshape(N, -1, f.h, f.w)[:, f.c_i:] == 0).all()
    if case == "unet_first_20x141":
        assert f.h > 2 * pad_y and f.w > 2 * pad_x
        mid = (slice(None), slice(None), slice(pad_y, f.h - pad_y), slice(pad_x, f.w - pad_x))
        assert torch.equal(dX[mid], before[mid]), "pixels outside the border bands must not be written"
        assert not torch.equal(dX, before)


@pytest.mark.parametrize("precision", list(PREC))
@pytest.mark.parametrize("case", list(CASES))
def test_frame_filter_gradient(case, precision):
    f = Frame(case, precision)
    o = f.o
    dws, db = f.wgrad()
    torch.cuda.synchronize()
    for name, dw in zip(f.L.LEARNED_FRAME_BANKS, dws):
        ref = o["grads"][name + ".weight"]
        a, r = tol("param", precision, ref)
        assert_close((dw.cpu().double() - 0.5), ref, a + 1e-6, r, f"{case} {precision} dW {name}")     # (+ the prefill's f32 rounding)
    a, r = tol("param", precision, o["db_frame"])
    assert_close(db.cpu().double() - 0.25, o["db_frame"], a + 1e-6, r, f"{case} {precision} dbias (frame share)")


@pytest.mark.parametrize("precision", list(PREC))
def test_frame_bit_reproducible(precision):
    f = Frame("deepest_8x31", precision)
    runs = []
    for _ in range(2):
        Y = f.forward()
        _, dX = f.dgrad()
        dws, db = f.wgrad()
        torch.cuda.synchronize()
        runs.append([Y, dX, db, *dws])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _engine_layer(case, counts=None):
    """One learned-padding layer through the engine (fp32): forward, backward; returns (engine, y, dx, grads, oracle)."""
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import engine as E
    c_i, c_o, k, symm, bc_x, bc_y, h, w = CASES[case]
    o = oracle(case, None)
    g = E.single_layer_graph(c_i, c_o, k, k // 2, "zeros", o["sym_h"], L.POST_NONE, "gelu", 1, False, learned=True, bc_x=bc_x,
                             bc_y=bc_y, input_grad=True)
    eng = E.Engine(g, "fp32")
    params = {n: t.float().contiguous().to(DEV) for n, t in o["sd"].items()}
    grads = {n: torch.zeros_like(t) for n, t in params.items()}
    x = o["x"].float().to(DEV)
    gout = o["ct"].float().to(DEV)
    eng.configure(N, h, w, torch.device(DEV))
    if counts is not None:
        counts.clear()
    y = eng.forward(x, params)
    eng.backward(gout, params, grads)
    torch.cuda.synchronize()
    return eng, y, from_cb8(eng.input_grad_cb8(), c_i), grads, o


@pytest.mark.parametrize("case", ["unet_first_20x141", "fluidnet_head_16x17"])
def test_whole_layer_through_engine(case):
    eng, y, dx, grads, o = _engine_layer(case)
    a, r = tol("y", "fp32", o["y"])
    assert_close(y.cpu().double(), o["y"], a, r, f"{case} engine y")
    a, r = tol("dx", "fp32", o["dx"])
    assert_close(dx, o["dx"], a, r, f"{case} engine dx")
    assert len(grads) == 10
    for n, gr in grads.items():
        ref = o["grads"][n]
        a, r = tol("param", "fp32", ref)
        assert_close(gr.cpu().double(), ref, a, r, f"{case} engine grad {n}")


FRAME_LAUNCHES = ("mc_learned_pack_banks_batched", "mc_learned_frame_fwd", "mc_learned_frame_dgrad", "mc_learned_frame_wgrad")


def _check_budget(counts):
    assert counts.get("mc_rect_copy", 0) <= 2, counts
    assert counts.get("mc_conv2d", 0) + counts.get("mc_conv2d_fused", 0) <= 2, counts
    assert counts.get("mc_conv2d_wgrad", 0) + counts.get("mc_conv2d_wgrad_fused", 0) <= 1, counts
    assert counts.get("mc_pack_weights", 0) == 0, counts
    for name in FRAME_LAUNCHES:
        assert counts.get(name, 0) == 1, (name, counts)


@pytest.fixture
def call_counts(monkeypatch):
    from pbml_mantle_convection_amd import _lib as L
    counts = {}
    real = L.call

    def counting(name, *args):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *args)

    monkeypatch.setattr(L, "call", counting)
    return counts


def test_launch_budget_engine(call_counts):
    _engine_layer("fluidnet_head_16x17", call_counts)
    _check_budget(call_counts)
    _engine_layer("unet_first_20x141", call_counts)          # (fx != fy: the main result is placed with one copy)
    _check_budget(call_counts)


def test_launch_budget_module(call_counts):
    from pbml_mantle_convection_amd.pytorch_networks_convae import BoundaryLearnedConvolution2D
    m = BoundaryLearnedConvolution2D(8, 16, 5, use_symm=True).to(DEV)
    x = torch.randn((N, 8, 12, 19), generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_(True)
    m(x)                                                      # (plans and allocates)
    call_counts.clear()
    y = m(x)
    y.sum().backward()
    torch.cuda.synchronize()
    _check_budget(call_counts)
    assert x.grad is not None and all(p.grad is not None for p in m.parameters())


@pytest.mark.parametrize("precision", list(PREC))
@pytest.mark.parametrize("case", ["deepest_8x31", "tiny_6x7", "k3_head_4x5"])
def test_module_on_engine(case, precision):
    """The stand-alone BoundaryLearnedConvolution2D is a one-node graph behind the autograd bridge: y, x.grad and the ten
    parameter gradients against the f64 oracle in every precision; bit-equal to an Engine driven by hand on the module's
    graph; bit-reproduced after the module re-planned for another shape; one in-flight forward per module."""
    from pbml_mantle_convection_amd import engine as E
    from pbml_mantle_convection_amd.pytorch_networks_convae import BoundaryLearnedConvolution2D
    c_i, c_o, k, symm, _, _, h, w = CASES[case]
    _, tx, tg = PREC[precision]
    o = oracle(case, None if precision == "fp32" else tx)
    m = BoundaryLearnedConvolution2D(c_i, c_o, k, use_symm=symm)
    m.load_state_dict({n: t.float() for n, t in o["sd"].items()})
    m = m.to(DEV).set_precision(precision)
    x = o["x"].float().to(DEV).requires_grad_(True)
    ct = o["ct"].float().to(DEV)

    def run():
        x.grad = None
        m.zero_grad()
        y = m(x)
        y.backward(ct)
        torch.cuda.synchronize()
        return [y.detach().clone(), x.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}]

    y, dx, grads = first = run()
    a, r = tol("y", precision, o["y"], stored=tx)
    assert_close(y.cpu().double(), o["y"], a, r, f"{case} {precision} module y")
    a, r = tol("dx", precision, o["dx"], stored=tg)
    assert_close(dx.cpu().double(), o["dx"], a, r, f"{case} {precision} module dx")
    assert len(grads) == 10
    for n, gr in grads.items():
        assert gr.shape == o["sd"][n].shape
        a, r = tol("param", precision, o["grads"][n])
        assert_close(gr.cpu().double(), o["grads"][n], a, r, f"{case} {precision} module grad {n}")
    # the same code gives the same bits: an engine on the module's graph, driven by hand
    eng = E.Engine(m._graph, precision)
    params = {n: p.detach() for n, p in m.named_parameters()}
    egrads = {n: torch.zeros_like(p) for n, p in params.items()}
    ey = eng.forward(x.detach(), params)
    eng.backward(ct, params, egrads)
    torch.cuda.synchronize()
    assert torch.equal(y, ey)
    assert torch.equal(dx.cpu().double(), from_cb8(eng.input_grad_cb8(), c_i))
    for n in grads:
        assert torch.equal(grads[n], egrads[n]), n
    # another shape re-plans the module's engine; back at the first shape the results are reproduced bit for bit
    x2 = torch.randn((N, c_i, h + 3, w + 3), generator=torch.Generator().manual_seed(9)).to(DEV)
    assert m(x2).shape == (N, c_o, h + 3, w + 3)
    y_b, dx_b, grads_b = run()
    assert torch.equal(y_b, y) and torch.equal(dx_b, dx)
    for n in grads:
        assert torch.equal(grads_b[n], grads[n]), n
    # a later forward overwrites the device activations of an earlier one
    stale = m(x)
    m(x)
    with pytest.raises(RuntimeError, match="one in-flight forward"):
        stale.backward(ct)

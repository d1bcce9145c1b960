"""The learned-padding frame kernels (csrc/conv_learned.hip) per element against f64, straight through the C ABI, at the
smallest shapes at which their index arithmetic can go wrong (tests/learned_cases.py: the case table, the f64 references from
oracle.ref_cpu.boundary_learned_conv and the per-element bound with K counted from the geometry;
tests/test_learned_cases_host.py: the table reaches what it was chosen for, the bounds hold for the operator in f32, the
comparisons have teeth).

  test_pack_*            bank layout bit for bit; 17 jobs in one call (two launches); dgrad_banks == NULL
  test_frame_forward     frame pixels per element, with and without bias; the interior untouched; lanes past c_out zero
  test_frame_input_gradient   dX prefilled with the main bank's gradient; lanes past c_in zero; pixels outside the bands untouched
  test_frame_filter_gradient  dW per bank and dbias onto exact prefills, NaN workspace; dbias == NULL changes no bit of dW
  test_two_runs_are_bit_identical

Every buffer a launch writes lies between two sentinel bands; the banks are prefilled with the byte 0xFF before packing (a
padding entry the pack kernel left unwritten would be a NaN the forward and input-gradient kernels multiply by zero); no
element is left out of any comparison.

Every test prints its worst err / tol (`pytest -s`).  On MI355X, worst case per kernel (f32 / bf16 / mix16):
  k_learned_frame_fwd     y 0.019 (group-seam) / 0.969 (band-seam) / 0.910 (band-seam);
                          bias == NULL 0.020 (band-seam) / 0.973 (first-layer) / 0.898 (minimal-k3)
  k_learned_frame_dgrad   dx 0.012 (tiles-k3) / 0.962 / 0.962 (long-row; mix16 is bf16 here)
  k_learned_frame_wgrad + k_learned_wgrad_reduce
                          dw 0.533 (minimal-k3: three visits, K + 1 = 4) / 0.247 / 0.247 (tiles-k3);
                          dbias 0.014 (minimal-k3) / 1.1e-4 / 1.1e-4 (band-seam)
  k_learned_pack          bit-equal
A 16-bit output sits just under 1 by construction: its error is the final rounding, at worst u |ref| of the u (|ref| + E) + E
allowed.  No ratio exceeded 1 and no kernel was changed."""
import ctypes as C

import pytest
import torch

import conv_variants as V
import learned_cases as Lc
from pbml_mantle_convection_amd import _lib as L
from test_hip_conv_variants import CB8, DEV, Guarded, assert_within, band, lanes

pytestmark = pytest.mark.gpu

INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
NAN = float("nan")


# ---- buffers --------------------------------------------------------------------------------------------------------------
def to_cb8(t, dtype):
    """NCHW (CPU, f64) -> CB8 [n][c8][h][w][8] in the storage type, the lanes past c zero."""
    n, c, h, w = t.shape
    c8 = (c + 7) // 8
    p = torch.zeros((n, c8 * CB8, h, w), dtype=torch.float64)
    p[:, :c] = t
    return p.view(n, c8, CB8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(dtype)


def on_device(t):
    """A CB8 tensor (CPU) inside a guarded device buffer."""
    g = Guarded(tuple(t.shape), t.dtype, band(t.shape[3], t.element_size()))
    g.t.copy_(t)
    return g


def bits(t):
    return t.contiguous().view(-1).view(torch.uint8).cpu()


def same_bits(a, b):
    return torch.equal(a.view(INT[a.dtype]), b.view(INT[b.dtype]))


class Weights:
    """The eight frame banks' unique filters on the device, and their pointer array."""

    def __init__(self, c):
        ws = Lc.inputs(c.id)[1]
        self.t = [ws[b].contiguous().to(DEV) for b in Lc.FRAME_BANKS]
        self.ptrs = [L.ptr(t) for t in self.t]


def empty_banks(c, dt):
    """(forward bank, input-gradient bank), every byte 0xFF, between sentinel bands."""
    d = Lc.desc(c, dt)
    out = []
    for dgrad in (0, 1):
        nbytes = L.call("mc_learned_bank_bytes", C.byref(d), dgrad)
        assert nbytes > 0
        out.append(Guarded((nbytes,), torch.uint8, 65536, fill=0xFF))
    return out


def packed_banks(c, dt):
    w = Weights(c)
    fwd, dg = empty_banks(c, dt)
    L.call("mc_learned_pack_banks_batched", C.byref(Lc.desc(c, dt)), (C.c_void_p * 8)(*w.ptrs), (C.c_void_p * 1)(fwd.ptr),
           (C.c_void_p * 1)(dg.ptr), 1, L.stream())
    torch.cuda.synchronize()
    fwd.assert_intact("forward bank")
    dg.assert_intact("input-gradient bank")
    return fwd, dg


def report(cid, dt, kernel, **ratios):
    print(f"\n[{cid} {dt}] {kernel}: worst err/tol " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


# ---- pack -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,dt", Lc.RUNS, ids=Lc.RUN_IDS)
def test_pack_layout_bit_for_bit(cid, dt):
    """Both banks, prefilled with 0xFF, against the numpy restatement of the layout: every element, the padding pairs,
    channels and rows (exact zeros) included."""
    L.load()
    c = Lc.CASE_BY_ID[cid]
    fwd, dg = packed_banks(c, dt)
    want_fwd, want_dg = Lc.bank_layout(c, dt)
    assert torch.equal(fwd.t.cpu(), bits(want_fwd)), "forward bank"
    assert torch.equal(dg.t.cpu(), bits(want_dg)), "input-gradient bank"


def test_pack_seventeen_jobs_in_one_call():
    """One job more than a launch takes, the case descriptors cycled in mixed precisions: job k is bit-equal to the same job
    packed alone (and so to the layout: test_pack_layout_bit_for_bit)."""
    L.load()
    jobs = [(Lc.FULL_CASES[k % len(Lc.FULL_CASES)], Lc.ALL[k % 3]) for k in range(17)]
    assert len(set(jobs)) == 17
    descs = (L.LearnedDesc * 17)(*[Lc.desc(c, dt) for c, dt in jobs])
    weights = [Weights(c) for c, _ in jobs]
    banks = [empty_banks(c, dt) for c, dt in jobs]
    L.call("mc_learned_pack_banks_batched", descs, (C.c_void_p * (17 * 8))(*[p for w in weights for p in w.ptrs]),
           (C.c_void_p * 17)(*[f.ptr for f, _ in banks]), (C.c_void_p * 17)(*[g.ptr for _, g in banks]), 17, L.stream())
    torch.cuda.synchronize()
    for k, ((c, dt), (fwd, dg)) in enumerate(zip(jobs, banks)):
        fwd.assert_intact(f"job {k} forward bank")
        dg.assert_intact(f"job {k} input-gradient bank")
        alone_fwd, alone_dg = packed_banks(c, dt)
        assert torch.equal(fwd.t, alone_fwd.t), (k, c.id, dt, "forward bank")
        assert torch.equal(dg.t, alone_dg.t), (k, c.id, dt, "input-gradient bank")
        want_fwd, want_dg = Lc.bank_layout(c, dt)
        assert torch.equal(fwd.t.cpu(), bits(want_fwd)) and torch.equal(dg.t.cpu(), bits(want_dg)), (k, c.id, dt)


@pytest.mark.parametrize("dt", Lc.ALL)
def test_pack_without_input_gradient_banks(dt):
    """dgrad_banks == NULL: the forward bank is complete and nothing is written past it."""
    L.load()
    c = Lc.CASE_BY_ID["tiles"]
    w = Weights(c)
    fwd, _ = empty_banks(c, dt)
    L.call("mc_learned_pack_banks_batched", C.byref(Lc.desc(c, dt)), (C.c_void_p * 8)(*w.ptrs), (C.c_void_p * 1)(fwd.ptr), None, 1,
           L.stream())
    torch.cuda.synchronize()
    fwd.assert_intact("forward bank")
    assert torch.equal(fwd.t.cpu(), bits(Lc.bank_layout(c, dt)[0]))


# ---- forward ----------------------------------------------------------------------------------------------------------------
def run_forward(c, dt, X, bank, bias):
    g = Lc.geometry(c.id)
    ft = V.FWD_T[dt]
    Y = Guarded((c.n, g.cbout, g.ho, g.wo, CB8), ft, band(g.wo, 4), fill=NAN)
    before = Y.t.clone()
    L.call("mc_learned_frame_fwd", C.byref(Lc.desc(c, dt)), X.ptr, bank.ptr, L.ptr(bias), Y.ptr, L.stream())
    torch.cuda.synchronize()
    for buf, what in ((Y, "y"), (X, "x"), (bank, "forward bank")):
        buf.assert_intact(what)
    return Y, before


@pytest.mark.parametrize("cid,dt", Lc.RUNS, ids=Lc.RUN_IDS)
def test_frame_forward(cid, dt):
    L.load()
    c = Lc.CASE_BY_ID[cid]
    g = Lc.geometry(cid)
    x, _, b, _ = Lc.inputs(cid)
    X = on_device(to_cb8(x.double(), V.FWD_T[dt]))
    bank, _ = packed_banks(c, dt)
    ratios = {}
    for what, bias in (("y", b.contiguous().to(DEV)), ("y_nobias", None)):
        ref = Lc.forward_ref(cid, dt, bias is not None)
        Y, before = run_forward(c, dt, X, bank, bias)
        full = lanes(Y)
        ratios[what] = assert_within(what, full[:, :c.co][:, :, g.frame], ref.y[:, :, g.frame], ref.tol[:, :, g.frame])
        assert bool((full[:, c.co:][:, :, g.frame] == 0).all()), "lanes past c_out of the frame are not zero"
        inner = (slice(None), slice(None), slice(g.fy, g.fy + g.mh), slice(g.fx, g.fx + g.mw))
        assert same_bits(Y.t[inner], before[inner]), "the interior rectangle was written"
    report(cid, dt, "k_learned_frame_fwd", **ratios)


# ---- input gradient -----------------------------------------------------------------------------------------------------------
def run_dgrad(c, dt, dY, dbank):
    ref = Lc.dgrad_ref(c.id, dt)
    dX = on_device(to_cb8(ref.before, ref.store))
    before = dX.t.clone()
    L.call("mc_learned_frame_dgrad", C.byref(Lc.desc(c, dt)), dY.ptr, dbank.ptr, dX.ptr, L.stream())
    torch.cuda.synchronize()
    for buf, what in ((dX, "dx"), (dY, "dy"), (dbank, "input-gradient bank")):
        buf.assert_intact(what)
    return dX, before


@pytest.mark.parametrize("cid,dt", Lc.RUNS, ids=Lc.RUN_IDS)
def test_frame_input_gradient(cid, dt):
    L.load()
    c = Lc.CASE_BY_ID[cid]
    g = Lc.geometry(cid)
    ref = Lc.dgrad_ref(cid, dt)
    dY = on_device(to_cb8(Lc.inputs(cid)[3].double(), V.GRAD_T[dt]))
    _, dbank = packed_banks(c, dt)
    dX, before = run_dgrad(c, dt, dY, dbank)
    full = lanes(dX)
    ratio = assert_within("dx", full[:, :c.ci], ref.dx, ref.tol)
    assert bool((full[:, c.ci:] == 0).all()), "lanes past c_in are not zero"
    outside = (g.readers == 0).to(DEV)
    assert same_bits(dX.t.permute(0, 1, 4, 2, 3)[..., outside], before.permute(0, 1, 4, 2, 3)[..., outside]), \
        "pixels outside the border bands were written"
    assert not same_bits(dX.t, before)
    report(cid, dt, "k_learned_frame_dgrad", dx=ratio, outside=int(outside.sum()))


# ---- filter gradient ------------------------------------------------------------------------------------------------------------
def run_wgrad(c, dt, X, dY, with_bias=True):
    g = Lc.geometry(c.id)
    d = Lc.desc(c, dt)
    nbytes = L.call("mc_learned_wgrad_workspace_bytes", C.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded((nbytes // 4,), torch.float32, 65536, fill=NAN)
    dws = [Guarded((g.u, c.ci, c.k, c.k), torch.float32, 65536, fill=Lc.DW_PREFILL[i]) for i in range(8)]
    db = Guarded((c.co,), torch.float32, 65536, fill=Lc.DB_PREFILL)
    L.call("mc_learned_frame_wgrad", C.byref(d), X.ptr, dY.ptr, ws.ptr, (C.c_void_p * 8)(*[t.ptr for t in dws]),
           db.ptr if with_bias else None, L.stream())
    torch.cuda.synchronize()
    for buf, what in [(ws, "workspace"), (db, "dbias"), (X, "x"), (dY, "dy")] + [(t, f"dw {b}") for t, b in zip(dws, Lc.FRAME_BANKS)]:
        buf.assert_intact(what)
    return dws, db


@pytest.mark.parametrize("cid,dt", Lc.WGRAD_RUNS, ids=Lc.WGRAD_RUN_IDS)
def test_frame_filter_gradient(cid, dt):
    L.load()
    c = Lc.CASE_BY_ID[cid]
    ref = Lc.wgrad_ref(cid, dt)
    x, _, _, ct = Lc.inputs(cid)
    X = on_device(to_cb8(x.double(), V.FWD_T[dt]))
    dY = on_device(to_cb8(ct.double(), V.GRAD_T[dt]))
    dws, db = run_wgrad(c, dt, X, dY)
    ratios = {}
    for t, bank in zip(dws, Lc.FRAME_BANKS):
        ratios[bank[5:]] = assert_within(f"dw {bank}", t.t.cpu(), *ref.dw[bank])
    ratios["dbias"] = assert_within("dbias", db.t.cpu(), ref.db, ref.db_tol)
    dws2, db2 = run_wgrad(c, dt, X, dY, with_bias=False)
    for t, t2, bank in zip(dws, dws2, Lc.FRAME_BANKS):
        assert same_bits(t.t, t2.t), f"dw {bank} differs without dbias"
    assert bool((db2.t == Lc.DB_PREFILL).all())
    report(cid, dt, "k_learned_frame_wgrad" + ("" if dt == "f32" else "_mfma"), dw=max(v for k, v in ratios.items() if k != "dbias"),
           dbias=ratios["dbias"])


# ---- reproducibility --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", Lc.ALL)
def test_two_runs_are_bit_identical(dt):
    L.load()
    c = Lc.CASE_BY_ID["tiles"]
    x, _, b, ct = Lc.inputs(c.id)
    X = on_device(to_cb8(x.double(), V.FWD_T[dt]))
    dY = on_device(to_cb8(ct.double(), V.GRAD_T[dt]))
    bias = b.contiguous().to(DEV)
    runs = []
    for _ in range(2):
        bank, dbank = packed_banks(c, dt)
        Y, _ = run_forward(c, dt, X, bank, bias)
        dX, _ = run_dgrad(c, dt, dY, dbank)
        dws, db = run_wgrad(c, dt, X, dY)
        runs.append([bank.t, dbank.t, Y.t, dX.t, db.t] + [t.t for t in dws])
    for a, b2 in zip(*runs):
        assert same_bits(a, b2) if a.dtype in INT else torch.equal(a, b2)

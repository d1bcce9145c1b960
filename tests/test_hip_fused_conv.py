"""The fused convolution launches against f64, straight through the C ABI, one launch chain per case (tests/fused_conv_cases.py:
the case tables, pinned to the dispatch by mc_conv_fused_kernel_name, the f64 references and the derived per-element bounds;
tests/test_fused_conv_cases_host.py checks tables, bounds and the teeth of the comparisons without a device).

  test_input_gradient_epilogue   mc_conv2d_fused with an mc_conv_epilogue, compared after the launch alone (final pixels dz,
                                 every other pixel of the padded buffer raw dA, slots 0 .. tiles - 1 the final region's sums,
                                 the slots behind them untouched), then mc_fold_padded_dz (the whole interior dz, all slots
                                 together the sums)
  test_apply_dz                  mc_gn_bwd_apply_dz per element, every source kind, and the identity without a table
  test_filter_gradient_from_dz   mc_gn_act_bwd_finalize_dz -> mc_conv2d_wgrad_dz -> finalize: the stored dY and (dW, db)
  test_conv_prologue             mc_conv2d_fused with an mc_conv_prologue (normalise on load)
  test_filter_gradient_prologue  mc_conv2d_wgrad_fused with one

Every buffer a launch writes lies between two sentinel bands that are checked afterwards, outputs are prefilled with NaN and
the inputs are surrounded by garbage, as in tests/test_hip_conv_variants.py.  The assertion is err <= tol with the derived tol
only; every test prints its worst err / tol (`pytest -s`).  On MI355X, worst case per instantiation (measured, not targets;
dz: final pixels of the conv launch, raw: its other pixels, fold: after mc_fold_padded_dz, S1 / S2: all slots):
  k_conv_direct_f32<5,dz> / <3,dz>             dz 0.063 / 0.037, raw 0.014 / 0.038, fold 0.063 / 0.045, S1 0.001 / 0.002
  k_conv_mfma_bf16<5,16,32,1,8,false,dz>       dz 0.782 (,h16: 0.939), raw 0.969 (0.952), fold 0.969 (0.952), S2 0.233 (0.182)
  k_conv_mfma_bf16<3,16,32,1,8,false,dz>       dz 0.899 (0.955), raw 0.981 (0.981), fold 0.960 (0.967), S2 0.239 (0.251)
  k_conv_mfma_bf16<5,8,16,2,2,false,dz>        dz 0.877 (0.841), raw 0.932 (0.953), fold 0.934 (0.953), S2 0.101 (0.068)
  k_conv_mfma_bf16<3,16,16,2,4,false,dz>       dz 0.968 (0.924), raw 0.977 (0.949), fold 0.977 (0.949), S1 0.066 (0.072)
  k_conv_rr_bf16<5,dz> / <3,dz>                dz 0.967 / 0.968, raw 0.973 / 0.982, fold 0.973 / 0.982, S2 0.029 / 0.011
  k_conv_rr_bf16<5,dz,act> / <3,dz,act>        dz 0.948 / 0.987, raw 0.971 / 0.982, fold 0.971 / 0.987, S2 5e-5 / 0.021
  k_conv_rr_bf16<5,dz,h16> / <3,dz,h16>        dz 0.965 / 0.966, raw 0.955 / 0.975, fold 0.965 / 0.975, S2 0.007 / 0.037
  k_conv_rr_bf16<5,dz,act,h16> / <3,...>       dz 0.935 / (no final pixel), raw 0.966 / 0.977, fold 0.948 / 0.974, S2 0.031 / 0.065
  k_conv_rr_bf16<5,dz,h16,dzm> / <3,...>       dz 0.925 / 0.956, raw 0.973 / 0.985, fold 0.973 / 0.979, S1 0.028 / 0.036,
                                               S2 0.047 / 0.044 (the stiff case: dz 0.925, S2 0.005)
  k_gn_bwd_apply_dz                            dy 0.996 (16-bit), 0.565 (f32), identity exact
  k_wgrad_mfma_bf16<DYZ>                       stored dY 0.996, dw 0.006, dbias 7e-5
  k_conv_direct_f32<5,norm> / <3,norm>         y 0.008 / 0.039
  k_conv_mfma_bf16<5,8,16,2,2,false,norm>      y 0.663 (,h16: 0.365);  <3,16,16,2,4,false,norm>: 0.968 (0.860)
  k_conv_rr_bf16<5,norm> / <3,norm>            y 0.708 / 0.603 (,h16: 0.302 / 0.225);  ,act: 0.762 / 0.991 (0.280 / 0.950)
  filter gradient with prologue                dw 0.053 (f32), 0.993 (16-bit, rr5-min-reflect-act: one flipped rounding of a
                                               staged value among 18 addends), dbias 0.026 / 2e-4
A stored 16-bit value sits just under 1 by construction (its error is the final rounding); the sums' bounds add every
pixel's worst case and sit far below 1: a missing, doubled or misplaced tile is far outside them, the last bits are not.  GELU
through the prologue sits lower than the other activations because its bound carries the polynomial's measured worst case at
every element."""
import ctypes as C

import pytest
import torch

import conv_variants as V
import fused_conv_cases as Fc
import gn_cases as G
from pbml_mantle_convection_amd import _lib as L
from test_hip_conv_variants import CB8, DEV, Guarded, assert_within, band, lanes, pack


def report(cid, kernel, **ratios):
    print(f"\n[{cid}] {kernel}: worst err/tol " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def packed_bank(d, w, dgrad):
    wd = w.to(DEV).contiguous()
    nbytes = L.call("mc_packed_weight_bytes", C.byref(d), dgrad)
    assert nbytes > 0
    b = Guarded((nbytes,), torch.uint8, 65536)
    L.call("mc_pack_weights", C.byref(d), L.ptr(wd), dgrad, b.ptr, L.stream())
    torch.cuda.synchronize()
    b.assert_intact("filter bank")
    return b


def check_sums(what, part, first, count, c, ref):
    """Slots [first, first + count) of the partial table, added in f64, against (S1, S2); the padded channels' entries are 0."""
    p = part.t.double().cpu()[:, first:first + count]
    assert bool(torch.isfinite(p).all()), f"{what}: a slot the launch owns was not written"
    assert bool((p[:, :, c:] == 0).all()), f"{what}: partials of the padded channels are not zero"
    s = p.sum(1)[:, :c]
    return (assert_within(what + " S1", s[..., 0], ref.s[..., 0], ref.tol[..., 0]),
            assert_within(what + " S2", s[..., 1], ref.s[..., 1], ref.tol[..., 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", Fc.EPI_IDS)
def test_input_gradient_epilogue(cid):
    L.load()
    c = Fc.EPI_BY_ID[cid]
    ops, ref = Fc.epi_operands(cid), Fc.epi_ref(cid)
    d, dd = Fc.epi_descs(c)
    dt = Fc.DT[c.prec]
    ft, gt = V.FWD_T[dt], V.GRAD_T[dt]
    p, (hs, ws), (hp, wp) = Fc.pad_of(c), c.hw, Fc.padded_hw(c)
    y = pack(ops.y, d.dtype, ft)
    dY = pack(ops.dY, dd.dtype, gt)
    bk = packed_bank(d, ops.w, 1)
    coef = ops.coef.to(DEV).contiguous() if c.coef else None
    tiles, fb = Fc.epi_slots(c)
    c8 = (c.c + 7) // 8
    buf = Guarded((c.n, c8, hp, wp, CB8), gt, band(wp), fill=float("nan"))
    part = Guarded((c.n, tiles + fb, c8 * CB8, 2), torch.float32, 65536, fill=float("nan"))
    epi = Fc.epilogue(c, y.ptr, L.ptr(coef), part.ptr)
    guarded = ((buf, "padded gradient buffer"), (part, "partials"), (y, "y"), (dY, "dY"), (bk, "filter bank"))

    L.call("mc_conv2d_fused", C.byref(dd), dY.ptr, None, None, bk.ptr, None, buf.ptr, None, None, C.byref(epi), L.stream())
    torch.cuda.synchronize()
    for g, what in guarded:
        g.assert_intact(what)
    got = lanes(buf)
    r_dz1 = assert_within("conv launch: final pixels", got[:, :c.c][:, :, ref.final], ref.stage1[:, :, ref.final],
                          ref.tol1[:, :, ref.final])
    r_raw = assert_within("conv launch: raw dA", got[:, :c.c][:, :, ~ref.final], ref.stage1[:, :, ~ref.final],
                          ref.tol1[:, :, ~ref.final])
    assert bool((got[:, c.c:] == 0).all()), "conv launch: lanes past the channel count are not zero"
    assert bool(torch.isnan(part.t[:, tiles:]).all()), "conv launch: a slot behind its tiles was written"
    r_s1, r_s2 = check_sums("conv launch", part, 0, tiles, c.c, ref.sums1)

    L.call("mc_fold_padded_dz", buf.ptr, c.n, c.c, hs, ws, p, L.PAD_MODES[c.mode], d.dtype, y.ptr, L.ptr(coef), L.ACTS[c.act],
           part.ptr, tiles + fb, tiles, L.stream())
    torch.cuda.synchronize()
    for g, what in guarded:
        g.assert_intact(what)
    got = lanes(buf)
    r_dz2 = assert_within("after the fold", got[:, :c.c], ref.stage2, ref.tol2)
    assert bool((got[:, c.c:] == 0).all()), "after the fold: lanes past the channel count are not zero"
    r_t1, r_t2 = check_sums("all slots", part, 0, tiles + fb, c.c, ref.sums2)
    report(cid, c.kernel, dz=r_dz1, raw=r_raw, S1=r_s1, S2=r_s2, dz_fold=r_dz2, S1_all=r_t1, S2_all=r_t2)


def grad_source(dz, c8, hw, pad, mode, gt):
    """The gradient source of a dz tensor (a packed Guarded CB8 buffer): MC_GSRC_PLAIN, or the interior of a padded buffer
    whose frame holds garbage (MC_GSRC_PADFOLD).  Returns (source, the buffer it points into)."""
    h, w = hw
    if not pad:
        return L.GradSrc(dz.ptr, L.GSRC_PLAIN, 0, 0, 1, h, w, 0, 0), dz
    buf = Guarded((dz.t.shape[0], c8, h + 2 * pad, w + 2 * pad, CB8), gt, band(w + 2 * pad), fill=G.GARBAGE)
    buf.t[:, :, pad:pad + h, pad:pad + w] = dz.t
    return L.GradSrc(buf.ptr, L.GSRC_PADFOLD, pad, L.PAD_MODES[mode], 1, h, w, 0, 0), buf


@pytest.mark.gpu
@pytest.mark.parametrize("cid", Fc.APPLY_IDS)
def test_apply_dz(cid):
    """mc_gn_bwd_apply_dz against dy = scale dz - rstd (m1 + yhat m2) in f64, per element; without a table the identity."""
    L.load()
    c = Fc.APPLY_BY_ID[cid]
    ops = Fc.apply_operands(cid)
    ref, tol = Fc.apply_ref(cid)
    dt = Fc.DT[c.prec]
    mc = V.MC[dt]
    mcg = L.MC_BF16 if mc == L.MC_MIX16 else mc
    ft, gt = V.FWD_T[dt], V.GRAD_T[dt]
    h, w = c.hw
    c8 = (c.c + 7) // 8
    y = pack(ops.y, mc, ft)
    gs, src = grad_source(pack(ops.dz, mcg, gt), c8, c.hw, c.pad, c.mode, gt)
    coef = ops.coef.to(DEV).contiguous() if c.gn else None
    m12 = ops.m12.to(DEV).contiguous() if c.gn else None
    dy = Guarded((Fc.N_B, c8, h, w, CB8), gt, band(w), fill=float("nan"))
    L.call("mc_gn_bwd_apply_dz", C.byref(gs), y.ptr, Fc.N_B, c.c, h, w, c.groups, L.ptr(coef), L.ptr(m12), mc, dy.ptr, L.stream())
    torch.cuda.synchronize()
    for g, what in ((dy, "dy"), (src, "dz"), (y, "y")):
        g.assert_intact(what)
    got = lanes(dy)
    ratio = assert_within("dy", got[:, :c.c], ref, tol)
    assert bool((got[:, c.c:] == 0).all()), "lanes past the channel count are not zero"
    report(cid, "k_gn_bwd_apply_dz", dy=ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", Fc.WDZ_IDS)
def test_filter_gradient_from_dz(cid):
    """mc_gn_act_bwd_finalize_dz -> mc_conv2d_wgrad_dz -> mc_conv2d_wgrad_finalize.  The dY the launch stores against the f64
    expression (m12 from the partials in f64), and (dW, db) against f64 sums of x and that stored dY, read back: the launch
    accumulates what it stores."""
    L.load()
    c = Fc.WDZ_BY_ID[cid]
    ops = Fc.wdz_operands(cid)
    d, _ = V.descs(Fc.wdz_layer(c), "mix16")
    h, w = c.hw
    co8 = (c.co + 7) // 8
    x = pack(ops.x, L.MC_MIX16, torch.float16)
    y = pack(ops.y, L.MC_MIX16, torch.float16)
    gs, src = grad_source(pack(ops.dz, L.MC_BF16, torch.bfloat16), co8, c.hw, c.zpad, c.mode, torch.bfloat16)
    part, gamma, coef = (t.to(DEV).contiguous() for t in (ops.part, ops.gamma, ops.coef))
    m12 = torch.zeros((Fc.N_B, c.groups, 2), device=DEV)
    dgamma, dbeta = torch.zeros(c.co, device=DEV), torch.zeros(c.co, device=DEV)
    tab = Guarded((Fc.N_B, co8 * CB8, 4), torch.float32, 4096, fill=0.0)
    L.call("mc_gn_act_bwd_finalize_dz", L.ptr(part), Fc.N_B, Fc.WDZ_BLOCKS, c.co, c.groups, h * w, L.ptr(gamma), L.ptr(m12),
           L.ptr(dgamma), L.ptr(dbeta), L.ptr(coef), tab.ptr, L.stream())
    dy = Guarded((Fc.N_B, co8, h, w, CB8), torch.bfloat16, band(w), fill=float("nan"))
    nbytes = L.call("mc_wgrad_partial_bytes", C.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded((nbytes // 4,), torch.float32, 65536, fill=float("nan"))
    L.call("mc_conv2d_wgrad_dz", C.byref(d), x.ptr, None, C.byref(gs), y.ptr, tab.ptr, dy.ptr, ws.ptr, L.stream())
    torch.cuda.synchronize()
    for g, what in ((tab, "dz_coef"), (dy, "dY"), (ws, "filter-gradient workspace"), (x, "x"), (y, "y"), (src, "dz")):
        g.assert_intact(what)
    got = lanes(dy)
    dy_ref, dy_tol = Fc.wdz_dy_ref(cid)
    r_dy = assert_within("dY", got[:, :c.co], dy_ref, dy_tol)
    assert bool((got[:, c.co:] == 0).all()), "dY: lanes past the channel count are not zero"
    dw = Guarded((c.co, c.ci, c.k, c.k), torch.float32, 65536, fill=V.WGRAD_PREFILL)
    db = Guarded((c.co,), torch.float32, 65536, fill=V.WGRAD_PREFILL)
    L.call("mc_conv2d_wgrad_finalize", C.byref(d), ws.ptr, dw.ptr, db.ptr, L.stream())
    torch.cuda.synchronize()
    for g, what in ((ws, "filter-gradient workspace"), (dw, "dw"), (db, "dbias")):
        g.assert_intact(what)
    dw_ref, dw_tol, db_ref, db_tol = Fc.wdz_wgrad_ref(cid, got[:, :c.co].double())
    r_w = assert_within("dw", dw.t.cpu(), dw_ref, dw_tol)
    r_b = assert_within("dbias", db.t.cpu(), db_ref, db_tol)
    report(cid, "k_wgrad_mfma_bf16<DYZ>", dY=r_dy, dw=r_w, dbias=r_b)


def pro_sources(c, dt):
    ops = Fc.pro_operands(c.id)
    xs = [pack(s, V.MC[dt], V.FWD_T[dt]) for s in ops.src]
    tabs = [t[dt].to(DEV).contiguous() if t[dt] is not None else None for t in ops.coef]
    while len(xs) < 2:
        xs.append(None), tabs.append(None)
    return xs, tabs, Fc.prologue(c, L.ptr(tabs[0]), L.ptr(tabs[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dt", Fc.PRO_RUNS, ids=Fc.PRO_RUN_IDS)
def test_conv_prologue(cid, dt):
    """mc_conv2d_fused with a prologue against conv(act(scale y0 + shift) | x1) in f64; the lanes past c_out exactly zero."""
    L.load()
    c = Fc.PRO_BY_ID[cid]
    ops = Fc.pro_operands(cid)
    d, _ = V.descs(Fc.pro_layer(c), dt)
    ref, tol = Fc.pro_forward_ref(cid, dt)
    (x0, x1), tabs, pro = pro_sources(c, dt)
    bk = packed_bank(d, ops.w, 0)
    bias = ops.b.to(DEV).contiguous()
    h, w = c.hw
    co8 = (c.co + 7) // 8
    y = Guarded((Fc.N_B, co8, h, w, CB8), V.FWD_T[dt], band(w), fill=float("nan"))
    L.call("mc_conv2d_fused", C.byref(d), x0.ptr, x1.ptr if x1 else None, C.byref(pro), bk.ptr, L.ptr(bias), y.ptr, None, None, None,
           L.stream())
    torch.cuda.synchronize()
    for g, what in ((y, "y"), (x0, "x0"), (x1, "x1"), (bk, "filter bank")):
        if g is not None:
            g.assert_intact(what)
    got = lanes(y)
    ratio = assert_within("y", got[:, :c.co], ref, tol)
    assert bool((got[:, c.co:] == 0).all()), "lanes past c_out are not zero"
    report(f"{cid} {dt}", Fc.pro_name(c, dt), y=ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dt", Fc.PRO_RUNS, ids=Fc.PRO_RUN_IDS)
def test_filter_gradient_prologue(cid, dt):
    """mc_conv2d_wgrad_fused with a prologue (workspace prefilled with NaN) + mc_conv2d_wgrad_finalize (accumulates onto 0.25)
    against f64 sums of the staged sources and the cotangent."""
    L.load()
    c = Fc.PRO_BY_ID[cid]
    ops = Fc.pro_operands(cid)
    d, dd = V.descs(Fc.pro_layer(c), dt)
    dw_ref, dw_tol, db_ref, db_tol = Fc.pro_wgrad_ref(cid, dt)
    (x0, x1), tabs, pro = pro_sources(c, dt)
    dy = pack(ops.ct, dd.dtype, V.GRAD_T[dt])
    nbytes = L.call("mc_wgrad_partial_bytes", C.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded((nbytes // 4,), torch.float32, 65536, fill=float("nan"))
    dw = Guarded(tuple(dw_ref.shape), torch.float32, 65536, fill=V.WGRAD_PREFILL)
    db = Guarded(tuple(db_ref.shape), torch.float32, 65536, fill=V.WGRAD_PREFILL)
    L.call("mc_conv2d_wgrad_fused", C.byref(d), x0.ptr, x1.ptr if x1 else None, C.byref(pro), dy.ptr, ws.ptr, L.stream())
    L.call("mc_conv2d_wgrad_finalize", C.byref(d), ws.ptr, dw.ptr, db.ptr, L.stream())
    torch.cuda.synchronize()
    for g, what in ((ws, "filter-gradient workspace"), (dw, "dw"), (db, "dbias"), (x0, "x0"), (x1, "x1"), (dy, "dy")):
        if g is not None:
            g.assert_intact(what)
    r_w = assert_within("dw", dw.t.cpu(), dw_ref, dw_tol)
    r_b = assert_within("dbias", db.t.cpu(), db_ref, db_tol)
    report(f"{cid} {dt}", "k_wgrad_mfma_bf16<PRO>" if dt != "f32" else "k_wgrad_direct_f32<PRO>", dw=r_w, dbias=r_b)

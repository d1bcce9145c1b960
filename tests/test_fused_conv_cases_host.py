"""Host-only checks of tests/fused_conv_cases.py (no device): every case reaches the instantiation written next to it
(mc_conv_fused_kernel_name), the shape rules the table was built by still hold, the DZM polynomial is what the kernel comment
says it is, and the comparisons of tests/test_hip_fused_conv.py have teeth."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import conv_variants as V
import fused_conv_cases as Fc
import gn_cases as G
from pbml_mantle_convection_amd import _lib as L


# ---- dispatch -------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_its_instantiation():
    """The name query takes the launch's own decisions (the h16 / GELU-only / DZM conditions are host functions both call), so a
    moved threshold -- CBin <= 2 for DZM, say -- shows here as a case that reached another instantiation."""
    reached = set()
    for c in Fc.EPI_CASES:
        assert Fc.epi_name(c) == c.kernel, (c.id, Fc.epi_name(c))
        reached.add(c.kernel)
    assert reached == Fc.EPI_KERNELS, reached ^ Fc.EPI_KERNELS
    reached = set()
    for cid, dt in Fc.PRO_RUNS:
        c = Fc.PRO_BY_ID[cid]
        want = c.kernel[:-1] + (",h16>" if dt == "mix16" else ">")
        assert Fc.pro_name(c, dt) == want, (cid, dt, Fc.pro_name(c, dt))
        reached.add(want)
    assert reached == Fc.PRO_KERNELS, reached ^ Fc.PRO_KERNELS


def test_name_query_without_fusion_is_the_plain_name():
    """Both pointers NULL, or a prologue with nothing to do: what mc_conv_kernel_name returns, for every descriptor of
    tests/conv_variants.py.  A launch the entry point would refuse has no name."""
    for cid, dt in V.RUNS:
        for d in V.descs(V.CASE_BY_ID[cid], dt):
            assert Fc.fused_name(d) == V.kernel_name(d)
            assert Fc.fused_name(d, pro=L.ConvPrologue(None, None, L.ACTS["none"], L.ACTS["none"])) == V.kernel_name(d)
    c = Fc.EPI_BY_ID["dzm5-seam"]
    dd = Fc.epi_descs(c)[1]
    epi = Fc.epilogue(c, Fc.P, Fc.P, Fc.P)
    assert Fc.fused_name(dd, pro=L.ConvPrologue(Fc.P, None, L.ACTS["gelu"], L.ACTS["none"]), epi=epi) == "unsupported"
    epi.hs += 1                                                          # (not the launch's padded domain)
    assert Fc.fused_name(dd, epi=epi) == "unsupported"
    epi = Fc.epilogue(c, None, Fc.P, Fc.P)                               # (no y)
    assert Fc.fused_name(dd, epi=epi) == "unsupported"


FAMILIES = {
    "direct": lambda c: c.prec == "f32",
    "wide": lambda c: c.kernel.startswith("k_conv_mfma_bf16"),
    "lex": lambda c: Fc.is_rr(c) and not Fc.is_dzm(c),
    "dzm": Fc.is_dzm,
}


def test_epilogue_table_follows_the_shape_rules():
    """The rules Table A was built by, so that a later edit keeps them."""
    lib = L.load()
    for fam, pred in FAMILIES.items():
        cs = [c for c in Fc.EPI_CASES if pred(c)]
        rr = fam in ("lex", "dzm")
        assert {c.mode for c in cs} == {"zeros", "replicate", "reflect"}, fam
        assert {c.k for c in cs} == {3, 5}, fam
        fr = Fc.frame_of
        # no final pixel / exactly one final row and column (row reuse: in the rows only -- its launches are >= 140 wide)
        assert any(fr(c) and c.hw[0] <= 2 * fr(c) and (rr or c.hw[1] <= 2 * fr(c)) for c in cs), fam
        assert any(fr(c) and c.hw[0] == 2 * fr(c) + 1 and (rr or c.hw[1] == 2 * fr(c) + 1) for c in cs), fam
        assert all(not Fc.epi_ref(c.id).final.any() for c in cs if fr(c) and c.hw[0] <= 2 * fr(c)), fam
        # the boundary of the final region strictly inside a tile, in both axes
        def inside(c):
            (th, tw), (y0, y1, x0, x1) = Fc.tile_of(c), Fc.final_box(c)
            return y1 > y0 and x1 > x0 and all(v % th for v in (y0, y1)) and all(v % tw for v in (x0, x1))
        assert any(inside(c) for c in cs), fam
        # padded size tile + 1 and 2 tile - 1 in both axes (row reuse: 3 tiles + 1 / - 1 wide)
        rel = [(Fc.padded_hw(c), Fc.tile_of(c)) for c in cs]
        assert any(s == (th + 1, (3 * tw if rr else tw) + 1) for s, (th, tw) in rel), fam
        assert any(s == (2 * th - 1, (3 if rr else 2) * tw - 1) for s, (th, tw) in rel), fam
        assert any(not c.coef for c in cs), fam
        if rr:
            # N x tiles above the work-group cap of rr_launch (256 / work-group columns): some work-groups walk two items
            big = [c for c in cs if c.n > 2]
            assert len(big) == 1, fam
            tiles = lib.mc_conv_tiles(C.byref(Fc.epi_descs(big[0])[1])) // 4           # (one slot per strip)
            cap = 256 // ((big[0].c + 15) // 16)
            assert cap < big[0].n * tiles < 2 * cap, (fam, big[0].n * tiles, cap)
            stiff = [c for c in cs if c.stiff]
            assert len(stiff) == 1, fam
            tab = Fc.epi_operands(stiff[0].id).coef.double()
            assert bool(((tab[:, 0, 2] * tab[:, 0, 3]).abs() - 8.0).abs().max() < 0.1), fam
    for c in Fc.EPI_CASES:
        assert c.c % c.groups == 0 and c.n >= 2
        if c.n == 2:
            hp, wp = Fc.padded_hw(c)
            assert hp <= 40 and wp <= 210, c.id
        assert Fc.is_rr(c) == (Fc.padded_hw(c)[1] >= 140 and c.prec != "f32"), c.id
        if Fc.is_dzm(c):
            assert c.prec == "mixed" and c.act == "gelu" and c.co <= 16, c.id
    assert {c.c for c in Fc.EPI_CASES} >= {10, 12, 20}
    assert {c.c // c.groups for c in Fc.EPI_CASES} == {1, 2, 4, 8}
    lex = [c for c in Fc.EPI_CASES if FAMILIES["lex"](c)]
    assert any(c.prec == "bf16" for c in lex) and any(c.prec == "mixed" and c.co > 16 for c in lex)
    assert any(c.act != "gelu" for c in lex) and any(c.act == "gelu" for c in lex)
    # DZM: the final region ends exactly on a tile edge -> some tiles take the unmasked path; one row less -> none does
    seam, less = Fc.EPI_BY_ID["dzm5-seam"], Fc.EPI_BY_ID["dzm5-seam-1"]
    assert less == seam._replace(id=less.id, hw=(seam.hw[0] - 1, seam.hw[1]))
    _, y1, _, x1 = Fc.final_box(seam)
    assert y1 % 16 == 0 and x1 % 64 == 0
    assert Fc.unmasked_tiles(seam) == [(1, 1), (1, 2)] and Fc.unmasked_tiles(less) == []
    assert Fc.unmasked_tiles(Fc.EPI_BY_ID["dzm5-stiff"]) and Fc.unmasked_tiles(Fc.EPI_BY_ID["dzm5-persistent"])


# ---- the DZM polynomial -----------------------------------------------------------------------------------------------------
def test_dzm_chain_restated_in_f16_lies_within_its_rounding_bound():
    """The numpy restatement of the kernel's f16 chain against the f64 evaluation of the same polynomial: within the running
    bound E_g, on a dense grid of z and on every DZM case's own z."""
    m = Fc.dzm_chain(np.linspace(-8.0, 8.0, 1_600_001))
    assert bool((np.abs(m.g16 - m.g) <= m.E).all()), float((np.abs(m.g16 - m.g) / m.E).max())
    worst = 0.0
    for c in Fc.EPI_CASES:
        if not Fc.is_dzm(c):
            continue
        ops = Fc.epi_operands(c.id)
        sc, sh, _, _ = Fc.coef_columns(c, ops.coef)
        m = Fc.dzm_model(V.rnd(ops.y, torch.float16).numpy(), sc.numpy(), sh.numpy())
        assert bool((np.abs(m.g16 - m.g) <= m.E).all()), c.id
        worst = max(worst, float((np.abs(m.g16 - m.g) / m.E).max()))
        if c.stiff:
            assert float(np.abs(m.z).max()) > 3.0                        # (the clamp is in play)
    print(f"\nDZM chain: worst |g16 - g| / E_g over the cases' own z {worst:.3f}")


def test_dzm_polynomial_against_erf_gelu_grad():
    """The f16 polynomial against erf-form GELU' in f64: no worse than the figures the kernel comment states (the erf form is
    the yardstick; the comment follows the measurement)."""
    src = open(os.path.join(G.ROOT, "pbml_mantle_convection_amd", "csrc", "conv_rr_bf16.hip")).read()
    m = re.search(r"rms error ([\d.e-]+) over z ~ N\(0, 1\), max ([\d.e-]+) in the tails", src)
    assert m, "the DZM comment no longer states its error figures"
    rms_c, max_c = float(m.group(1)), float(m.group(2))
    assert max_c <= 1.2e-2 and rms_c <= 1.7e-3
    emax, rms = Fc.dzm_vs_erf()
    print(f"\nDZM polynomial vs erf GELU': max {emax:.4e} over [-8, 8], rms {rms:.4e} over z ~ N(0, 1)")
    assert emax <= max_c and rms <= rms_c, (emax, rms)


# ---- the comparisons have teeth ----------------------------------------------------------------------------------------------
def _bad(c, value, ref, tol):
    return V.compare(Fc.stored_grad(c, value), ref, tol)[1]


@pytest.mark.parametrize("cid", Fc.EPI_IDS)
def test_epilogue_comparison_rejects_the_mutants(cid):
    """The reference rounded to the stored type passes both stages; a hole (NaN prefill) fails; each mutant fails -- frame width
    p instead of p + 1 at frame pixels only, act' at y, the neighbour's coefficient row, mean omitted from yhat."""
    c = Fc.EPI_BY_ID[cid]
    ops, r = Fc.epi_operands(cid), Fc.epi_ref(cid)
    p, (hs, ws) = Fc.pad_of(c), c.hw
    assert not _bad(c, r.stage1, r.stage1, r.tol1).any() and not _bad(c, r.stage2, r.stage2, r.tol2).any()
    hole = Fc.stored_grad(c, r.stage2)
    hole[-1, -1, p + hs - 1, p + ws - 1] = float("nan")
    assert int(V.compare(hole, r.stage2, r.tol2)[1].sum()) == 1
    tame = "the inputs are too tame"
    if c.mode != "zeros":
        m = Fc.epi_eval(c, ops, "frame_p")
        bad = _bad(c, m.stage1, r.stage1, r.tol1)
        frame = torch.zeros_like(r.final)
        frame[p:p + hs, p:p + ws] = True
        frame &= ~r.final
        assert bad.any(), "frame-width mutant passes after the conv launch: " + tame
        assert not bad[:, :, ~frame].any()
        if c.mode == "reflect":          # (replicate folds onto the edge pixel only: ring p is the same value either way)
            bad = _bad(c, m.stage2, r.stage2, r.tol2)
            assert bad.any(), "frame-width mutant passes after the fold: " + tame
            assert not bad[:, :, ~frame].any()
    if c.coef:
        for mutant in ("act_at_y", "next_row"):
            m = Fc.epi_eval(c, ops, mutant)
            assert _bad(c, m.stage2, r.stage2, r.tol2).any(), f"{mutant} mutant passes: " + tame
            if r.final.any():
                assert _bad(c, m.stage1, r.stage1, r.tol1)[:, :, r.final].any(), f"{mutant} mutant passes on the final pixels: " + tame
        m = Fc.epi_eval(c, ops, "next_row")
        assert V.compare(m.sums2.s, r.sums2.s, r.sums2.tol)[1].any(), "next_row mutant passes in the sums: " + tame
        m = Fc.epi_eval(c, ops, "no_mean")
        bad = V.compare(m.sums2.s, r.sums2.s, r.sums2.tol)[1]
        assert bad[..., 1].any() and not bad[..., 0].any(), "no_mean mutant passes: " + tame
        if r.final.any():
            assert V.compare(m.sums1.s, r.sums1.s, r.sums1.tol)[1][..., 1].any(), "no_mean mutant passes in the conv launch's slots: " + tame


# ---- Tables B and C ------------------------------------------------------------------------------------------------------------
def test_apply_and_filter_gradient_tables_follow_the_shape_rules():
    for prec in ("f32", "bf16", "mixed"):
        cs = [c for c in Fc.APPLY_CASES if c.prec == prec]
        assert {(c.pad, c.mode) for c in cs if c.gn} == set(Fc.APPLY_SOURCES), prec
        assert {c.c for c in cs} == {10, 12, 16} and {c.hw for c in cs} == set(Fc.APPLY_SIZES), prec
        assert sum(not c.gn for c in cs) == 1, prec
    assert all(c.c % c.groups == 0 for c in Fc.APPLY_CASES)
    w = Fc.WDZ_CASES
    assert {c.k for c in w} == {3, 5} and {c.zpad for c in w} == {0, 1, 2}
    assert {c.ci for c in w} == {10, 16} and {c.co for c in w} == {12, 16}
    assert {c.hw for c in w} >= {(16, 32), (17, 33), (31, 63)} and any(c.hw[0] < 16 and c.hw[1] < 32 for c in w)
    assert {c.mode for c in w} == {"zeros", "replicate", "reflect"}
    lib = L.load()
    for c in w:                                  # (the launch takes every case: MC_MIX16, one input chunk, one output group)
        assert c.co % c.groups == 0 and (c.ci + 7) // 8 <= 2 and c.co <= 16, c.id
        assert lib.mc_wgrad_partial_bytes(C.byref(V.descs(Fc.wdz_layer(c), "mix16")[0])) > 0


def test_prologue_table_follows_the_shape_rules():
    fams = {"direct": "k_conv_direct_f32", "wide": "k_conv_mfma_bf16", "rr": "k_conv_rr_bf16"}
    for fam, prefix in fams.items():
        cs = [c for c in Fc.PRO_CASES if c.kernel.startswith(prefix)]
        assert {c.k for c in cs} == {3, 5}, fam
        assert {c.mode for c in cs} == {"zeros", "replicate", "reflect"}, fam
        # coef on source 0 only beside a plain source 1 (the decoder pair); coef on both; activation without a table
        assert any(len(c.ci) == 2 and c.coefs == (True, False) and c.acts[1] == "none" for c in cs), fam
        assert any(c.coefs == (True, True) for c in cs), fam
        assert any(c.coefs == (False, False) and c.acts[0] != "none" for c in cs), fam
        assert any(c.acts[0] != "gelu" for c in cs) and any(c.acts[0] == "gelu" for c in cs), fam
        assert any(c.mode == "zeros" and c.coefs[0] for c in cs), fam              # (the okm mask)
        assert any(c.k == 5 and c.mode == "reflect" and c.hw == (3, 3) for c in cs), fam
        rel = [(c.hw, V.tile_of(c.kernel)) for c in cs]
        assert any(o == (th + 1, tw + 1) for o, (th, tw) in rel), fam
        assert any(o == (2 * th - 1, 2 * tw - 1) for o, (th, tw) in rel), fam
        assert any(o[0] < th and o[1] < tw for o, (th, tw) in rel), fam
    assert all(c.ci[0] % c.groups[0] == 0 and (len(c.ci) < 2 or c.ci[1] % c.groups[1] == 0) for c in Fc.PRO_CASES)
    # filter gradient: one and two co-tiles per block (an even number of 16-channel output tiles takes two)
    sixteen = [c for c in Fc.PRO_CASES if not c.f32]
    for k in (3, 5):
        assert {((c.co + 15) // 16) % 2 for c in sixteen if c.k == k} == {0, 1}, k


@pytest.mark.parametrize("cid", Fc.APPLY_IDS)
def test_apply_comparison_rejects_the_neighbouring_group(cid):
    c = Fc.APPLY_BY_ID[cid]
    ref, tol = Fc.apply_ref(cid)
    stored = lambda t: t.to(torch.float32).to(V.GRAD_T[Fc.DT[c.prec]]).double()      # noqa: E731
    assert not V.compare(stored(ref), ref, tol)[1].any()
    if c.gn:
        mutant, _ = Fc.apply_eval(c, Fc.apply_operands(cid), "next_group")
        assert V.compare(stored(mutant), ref, tol)[1].any(), "next_group mutant passes: the inputs are too tame"


@pytest.mark.parametrize("cid,dt", Fc.PRO_RUNS, ids=Fc.PRO_RUN_IDS)
def test_prologue_comparison_rejects_activated_padding(cid, dt):
    """The reference rounded to the stored type passes; with act(shift) in the zero-padded pixels it fails, within pad of the
    border only."""
    c = Fc.PRO_BY_ID[cid]
    y, tol = Fc.pro_forward_ref(cid, dt)
    stored = lambda t: t.to(torch.float32).to(V.FWD_T[dt]).double()      # noqa: E731
    assert not V.compare(stored(y), y, tol)[1].any()
    if c.mode == "zeros" and any(c.coefs):       # (without a table act(shift) = act(0) = 0: there is nothing to tell apart)
        mutant, _ = Fc.pro_forward_ref(cid, dt, "pad_act")
        bad = V.compare(stored(mutant), y, tol)[1]
        p = c.k // 2
        assert bad.any(), "pad_act mutant passes: the inputs are too tame"
        assert not bad[:, :, p:c.hw[0] - p, p:c.hw[1] - p].any()

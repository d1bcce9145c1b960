"""Host-only checks of tests/learned_cases.py (no device): the geometry every case was chosen for holds, recomputed from
engine.learned_regions and the library's size queries; the bounds are not too tight (the same operator in torch f32 on the CPU
lies within them at every element); and the comparisons of tests/test_hip_learned_kernels.py have teeth (every mutant of the
reference fails at one element or more).

test_mix16_filter_gradient_needs_the_second_rounding prints by how many bounds the filter gradient of x rounded to f16 ONLY
misses the f16-then-bf16 reference: 790 (band-seam) to 1.2e4 (minimal-k3) at these shapes, so it is asserted for every case."""
import ctypes as C
import os
import re

import pytest
import torch

import conv_variants as V
import gn_cases as G
import learned_cases as Lc
from oracle import ref_cpu as O
from pbml_mantle_convection_amd import _lib as L


def stored(t, ty):
    """A value as a kernel would leave it: f32, then the stored type."""
    return t.to(torch.float32).to(ty).double()


def ceil_div(a, b):
    return -(-a // b)


# ---- geometry -------------------------------------------------------------------------------------------------------------
def test_tables_geometry_is_the_librarys():
    """Bank sizes, slab counts and the validator, for every run: the table's numbers are the ones conv_learned.hip derives."""
    lib = L.load()
    for c in Lc.CASES:
        g = Lc.geometry(c.id)
        assert g.u == O.unique_filters(c.co, Lc.sym_dict(c))
        assert set(g.regs) == set(L.LEARNED_FRAME_BANKS)
        for dt in c.dts:
            d = Lc.desc(c, dt)
            es = 4 if dt == "f32" else 2
            assert lib.mc_learned_validate(C.byref(d)) == 0, (c.id, dt)
            assert lib.mc_learned_bank_bytes(C.byref(d), 0) == 8 * g.ct * g.jp * 128 * es, (c.id, dt)
            assert lib.mc_learned_bank_bytes(C.byref(d), 1) == 8 * g.it * g.jdp * 128 * es, (c.id, dt)
            total = sum(g.visits.values())
            smax = min(max((64 << 20) // Lc.slab_bytes(c), 8), 1024)
            sl = max(Lc.slmin(dt), ceil_div(total, smax))
            assert Lc.slabs(c, dt) == sum(ceil_div(v, sl) for v in g.visits.values()), (c.id, dt)
            assert (sl > Lc.slmin(dt)) == c.wgrad_only, (c.id, dt)


def test_every_case_reaches_what_it_was_chosen_for():
    G_ = Lc.geometry
    c, g = Lc.CASE_BY_ID["tiles"], G_("tiles")
    assert (g.ct, g.it) == (3, 2) and c.co % 16 == 8 and c.ci % 16 == 8 and c.n == 3
    assert g.sym_h == 10 and (g.j, g.jp, g.jd, g.jdp) == (75, 80, 125, 128)
    assert all((g.u + u) // 16 == 2 and u // 16 == 0 for u in range(g.nh))       # a copy lies in another tile than its source
    c, g = Lc.CASE_BY_ID["tiles-k3"], G_("tiles-k3")
    assert (g.ct, g.it) == (2, 3) and c.co % 16 == 8 and c.ci % 16 == 8 and (g.j, g.jp) == (45, 48) and c.bc_x != c.bc_y
    assert (g.u + 0) // 16 != 0                                                  # (here too: U = 21)
    c, g = Lc.CASE_BY_ID["first-layer"], G_("first-layer")
    assert c.bc_x == 4 and c.h == 2 * g.pad_y and c.w == 2 * g.pad_x + 1 and c.n == 3
    for cid in ("minimal-k5", "minimal-k3"):
        c, g = Lc.CASE_BY_ID[cid], G_(cid)
        assert (c.h, c.w) == (g.pad_y, g.pad_x) and bool((g.readers == 8).all())
        assert all(r[:4] == (0, 0, c.h, c.w) for r in g.regs.values())
        corner = (1, 1) if c.k == 3 else (2, 2)            # (the k = 5 strips are k + 1 wide: one output pixel at k = 3 only)
        assert all(g.regs[b][6:] == corner for b in g.regs if b.count("_") == 2)
    assert Lc.CASE_BY_ID["minimal-k3"].n == 3 and not Lc.CASE_BY_ID["minimal-k3"].symm
    for cid in ("group-seam", "band-seam"):
        c, g = Lc.CASE_BY_ID[cid], G_(cid)
        for b in ("conv_top", "conv_bottom"):
            rh, rw = g.regs[b][6:]
            assert (rh, rw) == (3, 11) and rh * rw % 16 == 1
            assert g.visits[b] % 2 == 1 and g.visits[b] % 8                      # a visit pair and an 8-visit lane half empty
        assert c.ci % 8 and c.co % 8 and c.n == 3 and not c.symm
    assert G_("band-seam").band_pix % 16 == 1
    # with bc_x = 1, as group-seam has it, no height gives band_pix = 1 mod 16: hence band-seam
    assert all((min(h, 14) * 15 + (h - min(h, 14)) * 12) % 16 != 1 for h in range(7, 1000))
    # the input gradient must leave the pixels outside the bands alone: some case has such pixels, some has none
    outside = {c.id for c in Lc.FULL_CASES if bool((G_(c.id).readers == 0).any())}
    assert "group-seam" in outside and "band-seam" not in outside
    for c in Lc.FULL_CASES:
        g = G_(c.id)
        assert int((g.readers > 0).sum()) == g.band_pix, c.id
    c, g = Lc.CASE_BY_ID["long-row"], G_("long-row")
    assert c.h < 2 * g.pad_y
    for b in ("conv_top", "conv_bottom"):
        assert ceil_div(g.visits[b], Lc.slmin("f32")) >= 9 and ceil_div(g.visits[b], Lc.slmin("bf16")) >= 5
        assert g.visits[b] % Lc.slmin("f32") and g.visits[b] % Lc.slmin("bf16")   # a partial last slice
    for cid, dt in (("slice-length-f32", "f32"), ("slice-length-16", "bf16"), ("slice-length-16", "mix16")):
        c, g = Lc.CASE_BY_ID[cid], G_(cid)
        assert Lc.slab_bytes(c) > 1_600_000 and (64 << 20) // Lc.slab_bytes(c) == 40
        assert sum(g.visits.values()) > 40 * Lc.slmin(dt)
        assert Lc.slabs(c, dt) < sum(ceil_div(v, Lc.slmin(dt)) for v in g.visits.values())
        # the smallest w at this n and h: with one column less the longer slices save no slab
        v = [c.n * 2 * (c.w - 1 - 4)] * 2 + [c.n * (c.h - 4) * 2] * 2 + [c.n * 4] * 4
        sl = max(Lc.slmin(dt), ceil_div(sum(v), 40))
        assert sum(ceil_div(b, sl) for b in v) == sum(ceil_div(b, Lc.slmin(dt)) for b in v)
    assert {dt for c in Lc.CASES if c.wgrad_only for dt in c.dts} == set(Lc.ALL)
    # the batched pack takes 16 jobs per launch: the GPU test's 17 jobs need a second one
    src = open(os.path.join(G.ROOT, "pbml_mantle_convection_amd", "csrc", "conv_learned.hip")).read()
    assert int(re.search(r"constexpr int LPK_MAX = (\d+);", src).group(1)) == 16


def test_restated_operator_and_strip_gradients_are_the_oracle():
    """The mutants' workbench (Lc.restated on explicit rectangles) is boundary_learned_conv; the strip-wise filter gradient of
    the slice-length cases is the whole operator's."""
    for c in Lc.FULL_CASES:
        x, ws, b, ct = Lc.inputs(c.id)
        x64, w64, b64 = x.double(), {n: w.double() for n, w in ws.items()}, b.double()
        y = Lc.operator(c, x64, w64, b64)
        assert torch.equal(Lc.restated(c, x64, Lc.full_banks(c, w64), b64), y), c.id
        whole, db = Lc.wg_eval(c, x64, ct.double())
        strips, dbs = Lc.wg_eval(c._replace(wgrad_only=True), x64, ct.double())
        assert torch.equal(db, dbs)
        for bank in Lc.FRAME_BANKS:
            assert bool(((whole[bank] - strips[bank]).abs() <= 1e-12 * (1 + whole[bank].abs())).all()), (c.id, bank)


# ---- the bounds are not too tight -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in Lc.FULL_CASES])
def test_bound_holds_for_the_operator_in_f32(cid):
    """The same operator in torch f32 on the CPU, on the f32 run's operands: within the bound at every element, forward and
    all gradients.  (Must pass before anything runs on a GPU.)"""
    c = Lc.CASE_BY_ID[cid]
    x, ws, b, ct = Lc.inputs(cid)
    r = Lc.forward_ref(cid, "f32")
    r_y, bad = V.compare(Lc.operator(c, x, ws, b), r.y, r.tol)
    assert not bad.any(), ("y", r_y)
    d = Lc.dgrad_ref(cid, "f32")
    _, frame = Lc.dx_eval(c, ws, ct)
    r_dx, bad = V.compare(d.before.float() + frame, d.dx, d.tol)
    assert not bad.any(), ("dx", r_dx)
    w = Lc.wgrad_ref(cid, "f32")
    dw, db = Lc.wg_eval(c, x, ct)
    r_dw = 0.0
    for i, bank in enumerate(Lc.FRAME_BANKS):
        ratio, bad = V.compare(dw[bank] + Lc.DW_PREFILL[i], *w.dw[bank])
        assert not bad.any(), ("dw", bank, ratio)
        r_dw = max(r_dw, ratio)
    r_db, bad = V.compare(db + Lc.DB_PREFILL, w.db, w.db_tol)
    assert not bad.any(), ("dbias", r_db)
    print(f"\n[{cid}] torch f32 on the CPU: worst err/tol y {r_y:.3g}, dx {r_dx:.3g}, dw {r_dw:.3g}, dbias {r_db:.3g}")


# ---- teeth ------------------------------------------------------------------------------------------------------------------
def _fwd_operands(cid, dt):
    c = Lc.CASE_BY_ID[cid]
    x, ws, b, _ = Lc.inputs(cid)
    ft = V.FWD_T[dt]
    return c, V.rnd(x, ft), {n: V.rnd(w, ft) for n, w in ws.items()}, b.double()


def _fwd_bad(cid, dt, mutant):
    r = Lc.forward_ref(cid, dt)
    return V.compare(stored(mutant, r.store), r.y, r.tol)[1]


TAME = "the inputs are too tame"


@pytest.mark.parametrize("dt", Lc.ALL)
def test_forward_comparison_rejects_the_mutants(dt):
    c, x64, w64, b64 = _fwd_operands("tiles", dt)
    g = Lc.geometry("tiles")
    r = Lc.forward_ref("tiles", dt)
    assert not _fwd_bad("tiles", dt, r.y).any()                                   # (the reference itself passes)
    hole = stored(r.y, r.store)
    hole[-1, -1, -1, -1] = float("nan")
    assert int(V.compare(hole, r.y, r.tol)[1].sum()) == 1
    full = Lc.full_banks(c, w64)

    def rect(bank):
        _, _, _, _, dy, dx, rh, rw = g.regs[bank]
        m = torch.zeros((g.ho, g.wo), dtype=torch.bool)
        m[dy:dy + rh, dx:dx + rw] = True
        return m

    # one bank's source strip shifted by one column
    regs = dict(g.regs, conv=g.main)
    sy, sx, sh, sw, dy, dx, rh, rw = regs["conv_left"]
    regs["conv_left"] = (sy, sx + 1, sh, sw, dy, dx, rh, rw)
    bad = _fwd_bad("tiles", dt, Lc.restated(c, x64, full, b64, regs))
    assert bad.any() and not bad[:, :, ~rect("conv_left")].any(), "shifted strip: " + TAME
    # the mirrored copies left unflipped
    bad = _fwd_bad("tiles", dt, Lc.restated(c, x64, Lc.full_banks(c, w64, unflipped=True), b64))
    assert bad[:, g.u:].any() and not bad[:, :g.u].any(), "unflipped copies: " + TAME
    # the weights of output tile 1 replaced by tile 0's (frame banks)
    mixed = {b: (w if b == "conv" else torch.cat([w[:16], w[:16], w[32:]], 0)) for b, w in full.items()}
    bad = _fwd_bad("tiles", dt, Lc.restated(c, x64, mixed, b64))
    assert bad[:, 16:32].any() and not bad[:, :16].any() and not bad[:, 32:].any(), "tile 0's weights in tile 1: " + TAME
    assert not bad[:, :, ~g.frame].any()
    # the bias omitted on the frame
    bad = _fwd_bad("tiles", dt, r.y - b64.view(1, -1, 1, 1) * g.frame)
    assert bad.any() and not bad[:, :, ~g.frame].any(), "bias omitted: " + TAME
    # left and right swapped
    c, x64, w64, b64 = _fwd_operands("first-layer", dt)
    g = Lc.geometry("first-layer")
    full = Lc.full_banks(c, w64)
    full["conv_left"], full["conv_right"] = full["conv_right"], full["conv_left"]
    bad = _fwd_bad("first-layer", dt, Lc.restated(c, x64, full, b64))
    sides = torch.zeros((g.ho, g.wo), dtype=torch.bool)
    for bank in ("conv_left", "conv_right"):
        _, _, _, _, dy, dx, rh, rw = g.regs[bank]
        sides[dy:dy + rh, dx:dx + rw] = True
    assert bad.any() and not bad[:, :, ~sides].any(), "left / right swapped: " + TAME


@pytest.mark.parametrize("dt", Lc.ALL)
def test_filter_gradient_comparison_rejects_the_mutants(dt):
    # one visit dropped: the last one of `top` (the partial last slice) and of a corner bank
    for cid, bank in (("long-row", "conv_top"), ("group-seam", "conv_bottom_left"), ("slice-length-f32", "conv_top")):
        if dt not in Lc.CASE_BY_ID[cid].dts:
            continue
        c, x64, ct64 = Lc.wgrad_operands(cid, dt)
        g = Lc.geometry(cid)
        ref, tol = Lc.wgrad_ref(cid, dt).dw[bank]
        assert not V.compare(ref, ref, tol)[1].any()
        rh, rw = g.regs[bank][6:]
        term = Lc.visit_term(c, bank, x64, ct64, c.n - 1, rh - 1, rw - 1)
        full = Lc.full_banks(c, {bank: torch.zeros_like(ref)})[bank] + term       # (the visit's term as a full-bank gradient)
        assert V.compare(ref - Lc.fold(c, full), ref, tol)[1].any(), f"{cid} {bank}: one visit dropped: " + TAME
    # the mirrored fold omitted
    c, x64, ct64 = Lc.wgrad_operands("tiles", dt)
    g = Lc.geometry("tiles")
    ctf, _ = Lc.split_ct(c, ct64)
    full = {b: torch.zeros((c.co, c.ci, c.k, c.k), dtype=torch.float64, requires_grad=True) for b in O.LEARNED_BANKS}
    (Lc.restated(c, x64, full, torch.zeros(c.co, dtype=torch.float64)) * ctf).sum().backward()
    w = Lc.wgrad_ref("tiles", dt)
    for i, bank in enumerate(Lc.FRAME_BANKS):
        ref, tol = w.dw[bank]
        assert not V.compare(Lc.fold(c, full[bank].grad) + Lc.DW_PREFILL[i], ref, tol)[1].any()
        bad = V.compare(full[bank].grad[:g.u] + Lc.DW_PREFILL[i], ref, tol)[1]
        assert bad[:g.nh].any() and not bad[g.nh:].any(), f"{bank}: fold omitted: " + TAME
    # one pixel's cotangent missing from the bias gradient
    db = w.db.clone()
    db -= ct64[0, :, 0, 0]
    assert V.compare(db, w.db, w.db_tol)[1].any(), "bias gradient: one pixel dropped: " + TAME


@pytest.mark.parametrize("dt", Lc.ALL)
def test_input_gradient_comparison_rejects_a_missing_bank(dt):
    """dX without one bank's share (the reader count K of the bound stays): fails inside that bank's source rectangle only."""
    c = Lc.CASE_BY_ID["minimal-k5"]
    _, ws, _, ct = Lc.inputs(c.id)
    gt = V.GRAD_T[dt]
    d = Lc.dgrad_ref(c.id, dt)
    assert not V.compare(stored(d.dx, d.store), d.dx, d.tol)[1].any()
    w64 = {n: V.rnd(w, gt) for n, w in ws.items()}
    w64["conv_top_right"] = torch.zeros_like(w64["conv_top_right"])
    _, frame = Lc.dx_eval(c, w64, V.rnd(ct, gt))
    assert V.compare(stored(d.before + frame, d.store), d.dx, d.tol)[1].any(), "one bank missing: " + TAME


def test_mix16_filter_gradient_needs_the_second_rounding():
    """MC_MIX16 converts x from f16 to bf16 on load.  A reference that rounds x to f16 only is another function: by how many
    bounds it differs, per case."""
    for c in Lc.CASES:
        if "mix16" not in c.dts:
            continue
        _, x16, ct64 = Lc.wgrad_operands(c.id, "mix16", xt=(torch.float16,))
        dw, _ = Lc.wg_eval(c, x16, ct64)
        w = Lc.wgrad_ref(c.id, "mix16")
        worst = max(V.compare(dw[b] + Lc.DW_PREFILL[i], *w.dw[b])[0] for i, b in enumerate(Lc.FRAME_BANKS))
        print(f"\n[{c.id}] x rounded to f16 only: worst err/tol of the filter gradient {worst:.3g}")
        assert worst > 1.0, c.id

"""CPU half of the layout / fold / copy / bicubic kernel tests (tests/glue_cases.py, tests/test_hip_glue_kernels.py): the references
are pinned to torch, the launch arithmetic the case table relies on is restated and checked against the figures the table was
built from, the refusals that are decided before any launch are called through the loaded library, the kink rule leaves at most
5 % of a fold_dz case out, and every mutant fails the very comparison function the GPU tests call -- while the comparison of
test_hip_parity.test_bicubic_adjoint_kernels_vs_torch lets one of them through."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import glue_cases as Gc

f64 = torch.float64
EINVAL, EUNSUP = -1, -2


# ---- the references, pinned to torch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [Gc.Bic(20, 24, 60, 72), Gc.Bic(24, 40, 12, 20)], ids=lambda b: b.tag)
def test_dense_bicubic_reference_is_interpolate(b):
    """out = Ty x Tx^T and dx = Ty^T g Tx from the engine's f32 tables against F.interpolate and its autograd in f64.  The tables
    are f32: a weight is off by U relatively, a product of two by 2 U, a merged transposed weight by one more."""
    x = Gc.randn((b.n, b.c, b.hi, b.wi), 1)
    xr = x.clone().requires_grad_(True)
    out = F.interpolate(xr, size=(b.ho, b.wo), mode="bicubic", align_corners=False)
    (Ty, Ay), (Tx, Ax) = Gc.dense_fwd(b.hi, b.ho), Gc.dense_fwd(b.wi, b.wo)
    Gc.compare(Gc.resample(x, Ty, Tx), out.detach(), Gc.gamma(3) * Gc.resample(x.abs(), Ay, Ax), "dense forward")
    g = Gc.randn(tuple(out.shape), 2)
    (dx,) = torch.autograd.grad(out, xr, g)
    Gc.compare(Gc.adjoint(g, Ty, Tx), dx, Gc.gamma(3) * Gc.adjoint(g.abs(), Ay, Ax), "adjoint from the forward tables")
    (Sy, By), (Sx, Bx) = Gc.dense_t(b.hi, b.ho), Gc.dense_t(b.wi, b.wo)
    Gc.compare(Gc.adjoint(g, Sy, Sx), dx, Gc.gamma(3) * Gc.adjoint(g.abs(), Ay, Ax), "adjoint from the transposed tables")
    assert bool((By <= Ay * (1 + 2 * Gc.U)).all()) and bool((Bx <= Ax * (1 + 2 * Gc.U)).all())      # |merged| <= merged |.|


@pytest.mark.parametrize("mode", Gc.FOLD_MODES)
@pytest.mark.parametrize("H,W,p", Gc.FOLD_CASES)
def test_fold_reference_is_the_adjoint_of_pad(H, W, p, mode):
    """The index-map form the mutants change equals autograd of F.pad, and <pad(x), g> = <x, fold(g)>."""
    gp = Gc.fold_inputs(H, W, p, "f32", c=8)
    a, b = Gc.fold_autograd(gp, p, mode), Gc.fold_index(gp, p, mode)
    assert float((a - b).abs().max()) <= 1e-14 * float(a.abs().max())
    x = Gc.randn((Gc.N, 8, H, W), 3)
    lhs, rhs = (F.pad(x, (p, p, p, p), mode=Gc.PAD_F[mode]) * gp).sum(), (x * a).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float((x.abs() * Gc.fold_autograd(gp.abs(), p, mode)).sum())
    cnt = Gc.fold_autograd(torch.ones_like(gp), p, mode)
    assert float(cnt.max()) <= 9 and not bool((cnt > 1)[:, :, ~Gc.frame_mask(H, W, p)].any())


def test_pool_and_mean_references():
    """unpool / 4 is the adjoint of F.avg_pool2d in floor mode; the pack_grad reference is autograd of crop(y - mean_HW(y))."""
    H, W = Gc.GSUM_HW
    for pool in (2, 3):
        a = torch.zeros((Gc.N, 16, H, W), dtype=f64, requires_grad=True)
        b = Gc.randn((Gc.N, 16, H // pool, W // pool), 4)
        F.avg_pool2d(a, pool).backward(b)
        assert float((a.grad - Gc.unpool(b, pool, H, W) / pool ** 2).abs().max()) <= 1e-15
        assert not bool(Gc.unpool(b, pool, H, W)[:, :, (H // pool) * pool:].any())
    c, (H, W, crop) = 3, Gc.UNPACK_SHAPES[0]
    g, _ = Gc.pack_grad_inputs(c, H, W, crop)
    y = Gc.randn((Gc.N, c, H, W), 5).requires_grad_(True)
    ((y - y.mean((2, 3), keepdim=True))[..., crop:W - crop] * g).sum().backward()
    assert float((y.grad - Gc.mean_grad_ref(g, H, W, crop)[0]).abs().max()) <= 1e-15


# ---- launch arithmetic ----------------------------------------------------------------------------------------------------------
def test_tap_list_lengths():
    """The figures of the case table, from engine.bicubic_tables."""
    for (a, b), taps in {(100, 128): 6, (200, 256): 6, (63, 127): 9, (24, 72): 12, (8, 32): 16, (32, 506): 64, (30, 60): 8, (20, 60): 12,
                         (65, 128): 8, (12, 24): 8, (64, 128): 8}.items():
        assert Gc.max_taps(a, b) == taps, (a, b, Gc.max_taps(a, b))
    # the four instantiations of k_bicubic_bwd, by (max_taps_y, max_taps_x)
    inst = [Gc.taps_launch(b)[2:] for b in Gc.TAPS_CASES[:4]]
    assert inst == [(8, 8), (8, 12), (12, 8), (12, 12)], inst
    assert Gc.max_taps(Gc.TAPS_GATHER.hi, Gc.TAPS_GATHER.ho) > 12                      # no slots: the per-pixel gather
    for b in Gc.SEP_CASES:
        assert b.ho // b.hi >= 4


def test_walk_strips_and_chunks():
    want = {(10, 100, 13, 128): (128, 64, 2, 8), (10, 65, 20, 128): (128, 61, 2, 8), (10, 200, 13, 256): (256, 128, 2, 8),
            (30, 63, 60, 127): (128, 63, 1, 12)}
    for b in Gc.WALK_CASES:
        SW, cw, strips, chunks, rpc, bxt = Gc.walk_launch(b)
        assert (SW, cw, strips, bxt) == want[(b.hi, b.wi, b.ho, b.wo)], (b.tag, SW, cw, strips, bxt)
        assert Gc.max_taps(b.wi, b.wo) <= 12
        # a strip's taps stay inside the block's SW columns (the kernel clamps silently if they do not)
        s, j = Gc.tables(b.wi, b.wo)[2:4]
        for X0 in range(0, b.wi, cw):
            X1 = min(b.wi, X0 + cw)
            assert int(j[s[X1] - 1]) - int(j[s[X0]]) < SW, (b.tag, X0)
    assert {Gc.walk_launch(b)[0] for b in Gc.WALK_CASES} == {128, 256}
    assert Gc.walk_launch(Gc.Bic(40, 300, 80, 600, Gc.N, 8))[0] == 512               # the instantiation the older test runs
    SW, cw, strips, chunks, rpc, bxt = Gc.walk_launch(Gc.WALK_LONG)
    assert (strips, chunks, rpc) == (1, 4, 16)                                      # long walks: 16 input rows, 32 output rows
    assert Gc.walk_launch(Gc.WALK_CASES[0])[4] <= 4                                 # ... against the 4 rows of the small cases
    SW, fw, strips, chunks, rpc = Gc.fwd_walk_launch(Gc.FWD_LONG)
    assert (strips, chunks, rpc) == (1, 4, 32)
    for b in Gc.FWD_DOWN:
        assert not Gc.fwd_takes_walk(b)                                             # k_bicubic_fwd, not the walk
    assert all(Gc.fwd_takes_walk(b) for b in Gc.FWD_OLD + Gc.FWD_ACT)
    # 24x40->12x20: 16 output rows span 32 input rows > FWH: bicubic_direct; 10x40->20x20: the rows fit, the columns do not
    b = Gc.FWD_DOWN[0]
    iy = Gc.tables(b.hi, b.ho)[0]
    assert int(iy[min(Gc.FOH, b.ho) - 1, 3]) - int(iy[0, 0]) >= Gc.FWH


def test_persistent_tiles_exceed_the_grid():
    tiles, grid, byt, bxt = Gc.taps_launch(Gc.TAPS_PERSISTENT)
    assert (tiles, grid) == (30, 24)
    for b in Gc.TAPS_CASES:
        t, g = Gc.taps_launch(b)[:2]
        assert t == g                                                               # the loop does not iterate anywhere else
    # the older test's largest case: 16 x 16 tiles against 768 blocks
    assert Gc.taps_launch(Gc.Bic(253, 256, 506, 512, Gc.N, 8))[:2] == (256, 256)


def test_fold_forms():
    forms = {(H, W, p): Gc.fold_shape(H, W, p) for H, W, p in Gc.FOLD_CASES}
    assert forms[(3, 9, 2)][0] == 1 and forms[(9, 3, 1)][0] == 1                    # `all`
    assert forms[(6, 7, 2)] == (0, 42, 0)                                           # hs == 2 (p + 1): no side bands
    assert forms[(5, 6, 1)][0] == 0 and forms[(5, 6, 1)][2] > 0 and forms[(7, 8, 2)][2] > 0
    assert forms[(40, 50, 2)][1] == 504 and Gc.fold_blocks(40, 50, 2) == 2
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    for (H, W, p) in Gc.FOLD_CASES:
        assert lib.mc_fold_blocks(H, W, p, L.PAD_MODES["reflect"]) == Gc.fold_blocks(H, W, p)
        assert int(Gc.frame_mask(H, W, p).sum()) == Gc.fold_shape(H, W, p)[1]
    assert lib.mc_fold_blocks(7, 8, 2, L.PAD_MODES["zeros"]) == 0 and lib.mc_fold_blocks(7, 8, 0, L.PAD_MODES["reflect"]) == 0


def test_sum_hw_paths():
    assert [Gc.sum_takes_vec(hw, 0) for hw in Gc.SUM_HW] == [False, False, True, True]
    assert not Gc.sum_takes_vec(64, 1)
    assert [Gc.k_sum(hw, Gc.sum_takes_vec(hw, 0)) for hw in Gc.SUM_HW] == [22, 22, 24, 25]
    assert Gc.k_sum(4100, False) == 26


# ---- refusals before any launch ---------------------------------------------------------------------------------------------------
def test_refusals_before_launch():
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    P = C.c_void_p(0x1000)
    R = L.PAD_MODES["reflect"]
    assert lib.mc_fold_padded(P, 2, 12, 7, 8, 3, R, L.MC_F32, None) == EINVAL
    assert lib.mc_fold_padded2(P, 8, P, 0, 2, 7, 8, 2, R, L.MC_F32, None) == EINVAL
    assert lib.mc_fold_padded2(P, 8, P, 12, 2, 7, 8, 3, R, L.MC_F32, None) == EINVAL
    assert lib.mc_fold_padded(P, 2, 12, 7, 8, 2, R, 99, None) == EUNSUP
    blocks = Gc.fold_blocks(7, 8, 2)
    assert lib.mc_fold_padded_dz(P, 2, 12, 7, 8, 2, R, L.MC_F32, P, None, L.ACTS["gelu"], P, Gc.DZ_FIRST + blocks - 1, Gc.DZ_FIRST, None) == EINVAL
    assert lib.mc_fold_padded_dz(P, 2, 12, 7, 8, 3, R, L.MC_F32, P, None, L.ACTS["gelu"], P, 9, 0, None) == EINVAL
    # a rectangle leaving the source, the destination
    (hs, ws), (hd, wd) = Gc.RECT_SRC, Gc.RECT_DST

    def rect(sy=2, sx=3, dy=1, dx=4, rh=5, rw=6, src=P):
        return lib.mc_rect_copy(src, hs, ws, sy, sx, P, hd, wd, dy, dx, rh, rw, 2, 12, 0, L.MC_F32, None)
    assert rect(sy=5) == EINVAL and rect(sx=6) == EINVAL and rect(dy=8) == EINVAL and rect(dx=8) == EINVAL
    assert rect(sy=-1) == EINVAL and rect(dx=-1) == EINVAL and rect(rh=0) == EINVAL
    assert rect(src=None, dy=8) == EINVAL
    # the walk adjoint
    b = Gc.WALK_CASES[0]
    gs = L.GradSrc(0x1000, L.GSRC_PLAIN, 0, 0, 1, b.ho, b.wo, 0, 0)

    def walk(g=gs, hi=b.hi, wi=b.wi, ho=b.ho, wo=b.wo, taps=6, dtype=L.MC_F32):
        return lib.mc_bicubic_bwd_walk(C.byref(g), 2, 12, hi, wi, ho, wo, P, P, P, P, P, P, P, taps, dtype, P, None)
    assert walk(taps=13) == EUNSUP and walk(taps=0) == EUNSUP
    assert walk(g=L.GradSrc(0x1000, L.GSRC_PLAIN, 0, 0, 1, 8, b.wo, 0, 0), hi=10, ho=8) == EINVAL           # ho < hi
    assert walk(g=L.GradSrc(0x1000, L.GSRC_PLAIN_POOL, 0, 0, 2, b.ho, b.wo, 0, 0)) == EUNSUP
    assert walk(g=L.GradSrc(0x1000, L.GSRC_PLAIN, 0, 0, 1, b.ho, b.wo, 4, 4)) == EINVAL                     # cb_off past the wide tensor
    assert lib.mc_bicubic_bwd_separable(C.byref(gs), 2, 12, b.hi, b.wi, b.ho, b.wo, P, P, P, P, P, P, L.MC_F32, None, P, None) == EINVAL
    assert lib.mc_bicubic_bwd_taps(C.byref(gs), 2, 12, b.hi, b.wi, b.ho + 1, b.wo, P, P, P, P, P, P, 8, 8, L.MC_F32, P, None) == EINVAL
    assert lib.mc_pack_nchw(P, 2, 3, 2, 5, 4, 0, 0, None, L.MC_F32, P, None) == EINVAL                      # src_c < c
    assert lib.mc_pack_nchw(P, 2, 3, 5, 5, 4, 4, R, None, L.MC_F32, P, None) == EINVAL                      # reflect needs pad_w < w
    assert lib.mc_unpack_nchw(P, 2, 3, 5, 6, 3, None, L.MC_F32, P, None) == EINVAL                          # nothing left of the width
    assert lib.mc_pack_grad_nchw(P, 2, 3, 5, 6, 3, None, L.MC_F32, P, None) == EINVAL
    assert lib.mc_sum_hw(P, 0, 4, 1.0, P, None) == EINVAL


# ---- the kink rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ("f32", "bf16", "mix16"))
@pytest.mark.parametrize("with_coef", (True, False))
@pytest.mark.parametrize("H,W,p", Gc.FOLD_CASES)
def test_kink_share_of_the_fold_dz_inputs(H, W, p, with_coef, prec):
    buf, y, coef = Gc.dz_inputs(H, W, p, prec, with_coef)
    r = Gc.dz_ref(buf, y, coef, p, "reflect", "relu", prec)
    assert float(r.kink.sum()) <= Gc.MAX_SHARE * float(r.frame.sum()) * buf.shape[0] * buf.shape[1]
    assert not bool(Gc.dz_ref(buf, y, coef, p, "reflect", "gelu", prec).kink.any())
    # the reference passes its own comparison after the store, and a fold that forgets the activation derivative does not
    after = buf.clone()
    after[:, :, p:p + H, p:p + W] = Gc.rq(r.dz, Gc.GRAD_DT[prec])
    Gc.check_fold_dz(buf, after, r.sums, y, coef, p, "reflect", "relu", prec, "reference")
    wrong = buf.clone()
    wrong[:, :, p:p + H, p:p + W] = Gc.rq(torch.where(r.frame, Gc.fold_autograd(buf, p, "reflect"), buf[:, :, p:p + H, p:p + W]), Gc.GRAD_DT[prec])
    with pytest.raises(AssertionError):
        Gc.check_fold_dz(buf, wrong, r.sums, y, coef, p, "reflect", "relu", prec, "dz without act'")


# ---- mutants --------------------------------------------------------------------------------------------------------------------------
MUT_WALK = Gc.WALK_CASES[0]                                     # 10x100 -> 13x128: two strips, every border row clamped
MUT_PERSISTENT = Gc.TAPS_PERSISTENT._replace(n=1, c=8)          # the persistent case's image and launch, one channel block of it


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("mutant", ("drop_merged", "seam_tap", "no_pad_offset", "no_cb_off"))
def test_walk_mutants_fail(mutant, dt):
    """1-4: a clamped border row's merged weight dropped; an x tap shifted by one at the strip seam; the PADFOLD offset ignored;
    the slice's cb_off ignored."""
    b = MUT_WALK._replace(dt=dt)
    Gc.check_adjoint(b, "walk", Gc.rq(Gc.adj_ref(b, "walk")[0], dt))
    with pytest.raises(AssertionError):
        Gc.check_adjoint(b, "walk", Gc.adj_mutant(b, "walk", mutant))


@pytest.mark.parametrize("kernel", ("taps", "separable"))
def test_other_adjoint_kernels_mutants_fail(kernel):
    b = Gc.TAPS_CASES[1]._replace(dt="bf16")
    Gc.check_adjoint(b, kernel, Gc.rq(Gc.adj_ref(b, kernel)[0], "bf16"))
    for mutant in ("no_pad_offset", "no_cb_off"):
        with pytest.raises(AssertionError):
            Gc.check_adjoint(b, kernel, Gc.adj_mutant(b, kernel, mutant))


def test_persistent_stale_origin_mutant_fails():
    """5: the second tile of a persistent block uses the first tile's window origin."""
    b = MUT_PERSISTENT
    Gc.check_adjoint(b, "taps", Gc.rq(Gc.adj_ref(b, "taps")[0], b.dt))
    with pytest.raises(AssertionError):
        Gc.check_adjoint(b, "taps", Gc.adj_mutant(b, "taps", "stale_origin", launch=Gc.TAPS_PERSISTENT))


@pytest.mark.parametrize("dt", ("f32", "bf16"))
@pytest.mark.parametrize("H,W,p,mode,mutant", [(7, 8, 2, "replicate", "no_diagonal"), (7, 8, 2, "reflect", "edge_mirror"),
                                               (5, 6, 1, "reflect", "edge_mirror"), (3, 9, 2, "reflect", "skip_last_row"),
                                               (9, 3, 1, "replicate", "skip_last_row")])
def test_fold_mutants_fail(H, W, p, mode, mutant, dt):
    """6-8: the replicate corner without its diagonal sources; the reflect mirror about the edge; the `all` form skipping the last
    row."""
    before = Gc.fold_inputs(H, W, p, dt)
    Gc.check_fold(before, Gc.fold_mutant_after(before, p, mode, dt, None), p, mode, dt, "reference")
    with pytest.raises(AssertionError):
        Gc.check_fold(before, Gc.fold_mutant_after(before, p, mode, dt, mutant), p, mode, dt, mutant)
    # in-place promises: a written halo, a written pixel outside the frame
    for y, x in ((0, 0), (p + H // 2, p + W // 2)):
        if (y, x) != (0, 0) and Gc.frame_mask(H, W, p)[y - p, x - p]:
            continue
        after = Gc.fold_mutant_after(before, p, mode, dt, None)
        after[0, 0, y, x] += 1.0
        with pytest.raises(AssertionError):
            Gc.check_fold(before, after, p, mode, dt, "written outside")


def test_converter_mutants_fail():
    """9, 10: the pack's reflect columns replicated; pack_grad leaving the cropped columns at zero."""
    (c, sc), (H, W, pad_w) = Gc.PACK_CHANNELS[0], Gc.PACK_SHAPES[0]
    x, cs = Gc.pack_inputs(c, sc, H, W)
    for dt in Gc.DT:
        Gc.check_pack(x, cs, c, pad_w, "reflect", dt, Gc.pack_ref(x, cs, c, pad_w, "reflect", dt), "reference")
        with pytest.raises(AssertionError):
            Gc.check_pack(x, cs, c, pad_w, "reflect", dt, Gc.pack_ref(x, cs, c, pad_w, "replicate", dt), "replicated")
        with pytest.raises(AssertionError):                      # the scale applied in f64, rounded once: not the kernel's two roundings
            Gc.check_pack(x, cs, c, 0, "zeros", "f32", Gc.from_cb8(Gc.to_cb8(x[:, :c] * cs.view(1, -1, 1, 1))), "unrounded product")
    c, (H, W, crop) = 3, Gc.UNPACK_SHAPES[0]
    g, mean = Gc.pack_grad_inputs(c, H, W, crop)
    for dt in ("f32", "bf16"):
        Gc.check_pack_grad(g, mean, c, crop, dt, Gc.pack_grad_ref(g, mean, c, crop, dt), "reference")
        with pytest.raises(AssertionError):
            Gc.check_pack_grad(g, mean, c, crop, dt, Gc.pack_grad_ref(g, mean, c, crop, dt, "crop_zero"), "crop_zero")
        m64 = F.pad(g, (crop, crop, 0, 0)).sum((2, 3)) / (H * W)
        got = Gc.pack_grad_ref(g, Gc.rq(m64, "f32"), c, crop, dt)
        Gc.check_pack_grad_mean(g, c, H, W, crop, dt, got)
        with pytest.raises(AssertionError):
            Gc.check_pack_grad_mean(g, c, H, W, crop, dt, Gc.pack_grad_ref(g, Gc.rq(m64, "f32"), c, crop, dt, "crop_zero"))


def test_rect_copy_and_gsrc_sum_mutants_fail():
    """11, 12: rect_copy ignoring `accumulate`; the pooled source adding the trailing odd row."""
    for dt in Gc.DT:
        src, dst = Gc.rect_inputs(dt)
        for r in Gc.RECTS:
            Gc.check_rect(src, dst, r, 1, dt, Gc.rect_ref(src, dst, r, 1, dt), "reference")
            with pytest.raises(AssertionError):
                Gc.check_rect(src, dst, r, 1, dt, Gc.rect_ref(src, dst, r, 1, dt, "no_accumulate"), "no_accumulate")
            assert torch.equal(Gc.rect_ref(None, dst, r, 1, dt), dst)                       # NULL source + accumulate: identity
    for dt in ("f32", "bf16"):
        for g1 in Gc.GSUM_G1[1:]:
            a, b = Gc.gsum_inputs(g1, dt)
            Gc.check_gsum(a, b, g1, dt, Gc.rq(Gc.gsum_ref(a, b, g1)[0], dt), "reference")
            with pytest.raises(AssertionError):
                Gc.check_gsum(a, b, g1, dt, Gc.rq(Gc.gsum_ref(a, b, g1, "trailing_row")[0], dt), "trailing_row")


def test_sum_and_forward_comparisons_reject_small_errors():
    """The remaining comparison functions: a sum that loses one value, a forward whose last row misses its merged weight."""
    x = Gc.randn((Gc.SUM_NC, 4100), 6)
    Gc.check_sum_hw(x, 0.5, True, Gc.rq(x.sum(1) * 0.5, "f32"), "reference")
    with pytest.raises(AssertionError):
        Gc.check_sum_hw(x, 0.5, True, Gc.rq(x[:, :-1].sum(1) * 0.5, "f32"), "one value short")
    for b in (Gc.FWD_DOWN[0], Gc.FWD_DOWN[3], Gc.Bic(5, 6, 10, 12)):
        xin = Gc.fwd_input(b)
        Gc.check_fwd(b, Gc.rq(Gc.fwd_ref(b)[0], b.dt))
        Ty = Gc.dense_fwd(b.hi, b.ho)[0].clone()
        Ty[-1, -1] *= 0.99
        with pytest.raises(AssertionError):
            Gc.check_fwd(b, Gc.rq(Gc.resample(xin, Ty, Gc.dense_fwd(b.wi, b.wo)[0]), b.dt))
    b = Gc.FWD_ACT[1]
    ref = Gc.fwd_act_ref(b, "gelu", True)[0]
    Gc.check_fwd_act(b, "gelu", True, Gc.rq(ref, b.dt))
    x, coef = Gc.fwd_act_inputs(b, True)
    with pytest.raises(AssertionError):                                                         # the affine forgotten
        Gc.check_fwd_act(b, "gelu", True, Gc.rq(Gc.resample(Gc.rq(F.gelu(x), b.dt), Gc.dense_fwd(b.hi, b.ho)[0], Gc.dense_fwd(b.wi, b.wo)[0]), b.dt))


def test_the_older_adjoint_comparison_lets_a_mutant_through():
    """The gap this closes: rtol = atol / max |ref| = 8e-3 (test_bicubic_adjoint_kernels_vs_torch, bf16) accepts the walk adjoint whose
    last output row skips its clamped tap; check_adjoint rejects it."""
    b = MUT_WALK._replace(dt="bf16")
    g = Gc.adj_input(b)
    x = torch.zeros((b.n, g.shape[1], b.hi, b.wi), dtype=f64, requires_grad=True)
    F.interpolate(x, size=(b.ho, b.wo), mode="bicubic", align_corners=False).backward(g)
    got = Gc.adj_mutant(b, "walk", "drop_merged")
    assert Gc.old_adjoint_comparison_passes(got, x.grad, "bf16")
    assert not Gc.old_adjoint_comparison_passes(Gc.adj_mutant(b, "walk", "seam_tap"), x.grad, "bf16")
    with pytest.raises(AssertionError):
        Gc.check_adjoint(b, "walk", got)

"""CPU: the f64 reference of the blurred-streamfunction heads (tests/blurr_ref.py) against the reference network's outputs (golden
g25), against its own expression through F.pad / F.conv2d and autograd, and against a 3 x 3 case computed by hand; what accepts
and what refuses the flag; and the mutants, each of which has to fail the comparison functions the GPU tests use, on their cases."""
import numpy as np
import pytest
import torch

import blurr_ref as R

CASES = [("wall", h, w) for (h, w) in R.WALL_SHAPES] + [("valid", h, w) for (h, w) in R.VALID_SHAPES]
GOLDEN = [("g25_newfluidnet_blurr", "wall"), ("g25_fluidnet_blurr", "valid")]


@pytest.mark.parametrize("name,form", GOLDEN)
def test_reference_equals_the_reference_network(golden, name, form):
    g = golden(name)
    u, v = R.head(form, g["y0"], float(g["a_bound"]))
    assert tuple(u.shape) == (1, 128, 506) and tuple(v.shape) == (1, 128, 506)
    worst = 0.0
    for got, want in R.golden_parts(g, u, v):
        worst = max(worst, float(np.abs(got - want).max()) / float(np.abs(want).max()))
        assert R.close64(got, want)
    print(f"\n{name}: largest |difference| / max |reference| {worst:.2e}")
    # the weight is the f32 value: with 1/9 in f64 the same comparison fails (the nine weights sum to 1 + 7.45e-9)
    u64, v64 = R.head(form, g["y0"], float(g["a_bound"]), "w64")
    assert not any(R.close64(got, want) for got, want in R.golden_parts(g, u64, v64))
    assert abs(9 * R.W32 - 1.0 - 7.45e-9) < 1e-11
    # and without the blur the outputs are others by far more than any tolerance of a network comparison
    import fields
    A = float(g["a_bound"]) * R.t64(g["y0"])
    u0 = R._diffs(A, False)[0]
    u0 = R._wall(u0, u0, False)[0] if form == "wall" else u0
    moved = float(np.abs(fields.strided_sample(u0.numpy(), 5003) - g["out/u"]).max()) / float(np.abs(g["out/u"]).max())
    print(f"  the blur moves u by up to {100 * moved:.1f} % of max |u|")
    assert moved > 0.02


@pytest.mark.parametrize("form,h,w", CASES)
def test_reference_equals_its_conv2d_restatement_and_autograd(form, h, w):
    c = R.case(form, h, w)
    y0 = R.t64(c["y"][:, 0]).requires_grad_(True)
    u, v = R.head(form, y0, c["ab"])
    cu, cv = R.head_conv2d(form, y0, c["ab"])
    scale = float(max(cu.detach().abs().max(), cv.detach().abs().max()))
    assert tuple(u.shape) == tuple(cu.shape) == (R.N, h, w)
    assert float((u - cu).detach().abs().max()) <= 1e-14 * scale and float((v - cv).detach().abs().max()) <= 1e-14 * scale
    ((cu * R.t64(c["gu"])).sum() + (cv * R.t64(c["gv"])).sum()).backward()
    ga = R.head_adj(form, c["gu"], c["gv"], c["ab"])
    assert float((ga - y0.grad).abs().max()) <= 1e-14 * float(y0.grad.abs().max())
    # the reference passes its own comparison functions with nothing to spare, and the identity holds
    assert R.fwd_ratio(c, u.detach(), v.detach()) == 0.0 and R.bwd_ratio(c, ga) == 0.0
    assert R.identity_ratio(c, u.detach(), v.detach(), ga) < 1e-6
    if form == "wall":
        for t in (u, v):
            assert all(float(t[n, i, j]) == 0.0 for n in range(R.N) for i in (0, -1) for j in (0, -1))
    # the magnitudes bound the values
    mu, mv = R.head(form, y0.detach(), c["ab"], mag=True)
    assert bool((mu >= u.detach().abs() - 1e-14).all()) and bool((mv >= v.detach().abs() - 1e-14).all())
    assert bool((R.head_adj(form, c["gu"], c["gv"], c["ab"], mag=True) >= ga.abs() - 1e-14).all())


def test_hand_computed_3x3():
    """A = [[9, 0, 0], [0, 0, 0], [0, 0, 18]] with a_bound = 1 and w = W32: the clamp counts A[0][0] four times in B[0][0], twice in
    B[0][1] and B[1][0], once in B[1][1], and A[2][2] likewise from the other corner."""
    w = R.W32
    y0 = np.array([[[9.0, 0, 0], [0, 0, 0], [0, 0, 18.0]]])
    B = R.box_mean(y0).numpy()[0]
    want = w * np.array([[36.0, 18, 0], [18, 27, 36], [0, 36, 72]])
    np.testing.assert_allclose(B, want, rtol=0, atol=1e-14)
    # wall form on 3 x 3: the one interior value u_in = 0.5 (B[2][1] - B[0][1]) = 9 w, v_in = -0.5 (B[1][2] - B[1][0]) = -9 w;
    # u: the wall columns are corners (0) or the negated middle row; v: the wall rows likewise
    u, v = R.head("wall", y0, 1.0)
    np.testing.assert_allclose(u.numpy()[0], 9 * w * np.array([[0.0, 1, 0], [-1, 1, -1], [0, 1, 0]]), rtol=0, atol=1e-14)
    np.testing.assert_allclose(v.numpy()[0], -9 * w * np.array([[0.0, -1, 0], [1, 1, 1], [0, -1, 0]]), rtol=0, atol=1e-14)
    # valid form on the same plane: one pixel
    u, v = R.head("valid", y0, 2.0)
    assert abs(float(u) - 18 * w) < 1e-14 and abs(float(v) + 18 * w) < 1e-14 and tuple(u.shape) == (1, 1, 1)
    # adjoint of the valid form for gu = 1, gv = 0, a_bound = 2: gB[2][1] = 0.5, gB[0][1] = -0.5; row 0 of ga takes
    # 2 gB[0] + gB[1] = -1 in each of its three columns, row 1 takes gB[0] + gB[1] + gB[2] = 0, row 2 mirrors row 0
    ga = R.head_adj("valid", np.ones((1, 1, 1)), np.zeros((1, 1, 1)), 2.0).numpy()[0]
    np.testing.assert_allclose(ga, w * np.array([[-2.0, -2, -2], [0, 0, 0], [2, 2, 2]]), rtol=0, atol=1e-14)


@pytest.mark.parametrize("form,h,w", CASES)
def test_every_mutant_fails_the_comparison_functions(form, h, w):
    c = R.case(form, h, w)
    y0 = c["y"][:, 0]
    u, v = R.head(form, y0, c["ab"])
    ga = R.head_adj(form, c["gu"], c["gv"], c["ab"])
    for mutant in R.MUTANTS:
        mu, mv = R.head(form, y0, c["ab"], mutant)
        mg = R.head_adj(form, c["gu"], c["gv"], c["ab"], mutant)
        rf, rb = R.fwd_ratio(c, mu, mv), R.bwd_ratio(c, mg)
        ri = R.identity_ratio(c, mu if mutant != "adj_ny1" else u, mv if mutant != "adj_ny1" else v, mg if mutant == "adj_ny1" else ga)
        print(f"\n{form} {h}x{w} {mutant}: forward {rf:.3g}, adjoint {rb:.3g}, identity (one side mutated) {ri:.3g}")
        if mutant == "adj_ny1":                             # (a mutant of the adjoint alone: its forward is the reference's)
            assert rf == 0.0 and rb > 1.0 and ri > 1.0
        else:
            assert rf > 1.0 and rb > 1.0 and ri > 1.0


def test_what_accepts_the_flag_and_what_refuses_it():
    from pbml_mantle_convection_amd.losses import StokesLoss
    from pbml_mantle_convection_amd.pytorch_networks_convae import ConvAE, FluidNet, NewFluidNet, Unet
    for lt in ("curl", "mae", "mass"):                      # ('mae' / 'mass': accepted and never read, as in the reference)
        on = NewFluidNet(2, 7, 8, 3, None, "gelu", "replicate", lt, repeats=1, blurr=True)
        off = NewFluidNet(2, 7, 8, 3, None, "gelu", "replicate", lt, repeats=1)
        assert off.blurrer is None and tuple(on.blurrer.shape) == (1, 1, 3, 3) and on.blurrer.dtype == torch.float32
        assert bool((on.blurrer.double() == R.W32).all())
        assert list(on.state_dict()) == list(off.state_dict()) and not any("blurr" in k for k in on.state_dict())
    on = FluidNet(2, 7, 8, 1, None, "gelu", "learned", "curl", repeats=1, f=5, p_pred=False, blurr=True)
    off = FluidNet(2, 7, 8, 1, None, "gelu", "learned", "curl", repeats=1, f=5, p_pred=False)
    assert off.blurrer is None and bool((on.blurrer.double() == R.W32).all()) and list(on.state_dict()) == list(off.state_dict())
    with pytest.raises(NotImplementedError, match="sigma is drawn at random"):
        Unet(2, 10, 8, 3, None, "gelu", "replicate", "curl", repeats=1, blurr=True)
    with pytest.raises(NotImplementedError, match="blurr"):
        ConvAE(1, 10, 8, 3, None, "gelu", "replicate", "mae", repeats=1, blurr=True)
    assert StokesLoss(True, "curl", has_T=False, blurr=True).blurr and not StokesLoss(True, "curl", has_T=False).blurr
    assert StokesLoss(False, "curl", has_T=False, curl_valid=True, blurr=True).blurr
    with pytest.raises(ValueError, match="blurr"):
        StokesLoss(True, "curl", blurr=True)                # the Unet's head (has_T)
    for lt in ("mae", "mass"):
        with pytest.raises(ValueError, match="blurr"):
            StokesLoss(True, lt, has_T=False, blurr=True)


def test_command_lines_and_run_name():
    from pbml_mantle_convection_amd import evaluate as E
    from pbml_mantle_convection_amd import multigpu as G
    from pbml_mantle_convection_amd import rollout as Ro
    a = G.build_arg_parser().parse_args(["-blurr", "1", "-f", "8", "-b", "2", "-s", "0", "-ab", "10", "-r", "1", "-k", "3"])
    assert a.blurr == 1 and G.run_name(a).endswith("_blurr")
    assert "_blurr" not in G.run_name(G.build_arg_parser().parse_args(["-f", "8", "-b", "2", "-s", "0", "-ab", "10", "-r", "1", "-k", "3"]))
    r = Ro.build_arg_parser().parse_args(["--params", "p.csv", "--steps", "1", "--out", "o", "-lt", "curl", "-blurr", "1"])
    assert r.blurr == 1 and Ro.build_arg_parser().parse_args(["--params", "p.csv", "--steps", "1", "--out", "o"]).blurr == 0
    e = E.build_arg_parser().parse_args(["--out", "o", "-lt", "curl", "-blurr", "1"])
    assert e.blurr == 1 and E.build_arg_parser().parse_args(["--out", "o"]).blurr == 0

"""CPU-only checks of tests/loss_cases.py, the harness of tests/test_hip_loss_kernels.py: the f64 restatements equal the oracle at
ra = 1, inv_h = 126; the kink rules leave out at most 5 % of any case; every mutant of the reference fails the comparison functions
the GPU tests use; and the momentum check of tests/test_hip_train.py, restated, passes the first two mutants."""
import numpy as np
import pytest
import torch

import fields
import loss_cases as Lc
from oracle import ref_cpu as O

f64 = torch.float64
ALL_SHAPES = [(Lc.B, H, W) for H, W in Lc.SHAPES]
TYPE_NAME = {0: "mae", 1: "mass", 2: "curl"}


def test_restatement_equals_the_oracle():
    for N, H, W in ALL_SHAPES:
        d = Lc.inputs(N, H, W)
        eta = O.viscosity(d["T"], d["yc"], d["paras"])
        mine = Lc.eta64(d["T"], d["yc"], d["paras"])[0]
        assert torch.allclose(mine, eta, rtol=1e-7, atol=0)              # (the lower clip is f32(1e-8) here: 6e-9 away)
        rx, ry = O.momentum_residual(d["u"], d["v"], d["p"], d["T"], d["yc"], d["paras"], d["scaler"])
        mx, my = Lc.residual64(d["u"], d["v"], d["p"], d["T"], eta, d["scaler"], ra=O.RA, ih=O.INV_H)
        for a, b in ((mx, rx), (my, ry)):
            assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
        for _, p_pred, lt, ls, ld, l2, t_grad in Lc.FLAG_CASES:
            ch = [0, 1] + ([2] if p_pred else []) + ([3] if t_grad >= 0 else [])
            truth = d["truth"][:, ch]
            kw = dict(p_pred=p_pred, loss_type=TYPE_NAME[lt], loss_scale=ls, loss_derivative=ld, norm="l2" if l2 else "l1")
            p = d["p"] if p_pred else None
            ref = (O.get_loss_unet((d["u"], d["v"], p, d["T"]), truth, **kw) if t_grad >= 0
                   else O.get_loss_fluidnet((d["u"], d["v"], p), truth, **kw))
            terms, out6 = Lc.stokes_terms64(d["u"], d["v"], d["p"], d["T"], truth, p_pred=p_pred, loss_type=lt, ls=ls, ld=ld, l2=l2,
                                            has_T=t_grad >= 0)
            for a, b in zip(out6, ref):
                assert abs(float(a) - float(b)) <= 1e-12 * max(1.0, abs(float(b))), (H, W, kw, float(a), float(b))
    for H, W in Lc.CURL_SHAPES:
        a = Lc.curl_case(H, W)["a"]
        u, v = Lc.curl_head64(a)
        ru, rv = O.curl_head(a.unsqueeze(1))
        assert torch.equal(u, ru[:, 0]) and torch.equal(v, rv[:, 0])


def test_viscosity_clips_at_both_ends():
    d = Lc.inputs(Lc.B, 17, 65)
    eta, rel, e = Lc.eta_error(d["T"], d["yc"], d["paras"])
    assert bool((eta == Lc.ETA_LO).any()) and bool((eta == 1.0).any()) and bool(((eta > Lc.ETA_LO) & (eta < 1.0)).any())
    assert bool((e == 0).any()) and bool((e > 0).any())
    assert len(set(d["scaler"].tolist())) == Lc.B


def _grad_cases():
    for N, H, W in ALL_SHAPES + [Lc.MANY]:
        yield "C", (N, H, W), dict(p_pred=True, loss_type=0, ls=False, ld=False, l2=False, t_grad=1, lam=1.0)
    for N, H, W in ALL_SHAPES:
        for _, p_pred, lt, ls, ld, l2, t_grad in Lc.FLAG_CASES:
            yield "D", (N, H, W), dict(p_pred=p_pred, loss_type=lt, ls=ls, ld=ld, l2=l2, t_grad=t_grad)


def test_kink_rules_leave_out_at_most_five_percent():
    """F1: from the reference alone.  The cap is a condition on the inputs."""
    worst = {}
    for N, H, W in ALL_SHAPES + [Lc.MANY]:
        r = Lc.Residual(Lc.inputs(N, H, W), 1e-6)
        worst["B"] = max(worst.get("B", 0.0), r.share())
        assert r.share() <= Lc.MAX_SHARE, ("B", H, W, r.share())
    for part, (N, H, W), kw in _grad_cases():
        d = Lc.inputs(N, H, W)
        truth = torch.stack([d["u"], d["v"], d["p"], d["T"]], 1) if part == "C" else None
        g = Lc.StokesGrad(d, truth=truth, **kw)
        worst[part] = max(worst.get(part, 0.0), g.share)
        assert g.share <= Lc.MAX_SHARE, (part, H, W, kw, g.share)
    print("\nlargest share left out: " + ", ".join(f"part {k} {v:.4f}" for k, v in sorted(worst.items())))


def _adjoint_mutants(c):
    ref, sx, sy, eta, s = c["ref"], c["sx"], c["sy"], c["eta"], c["s"]
    z = torch.zeros_like(ref[0])
    return {
        "dP dropped": [ref[0], ref[1], z, ref[3]],
        "the buoyancy adjoint dropped": [ref[0], ref[1], ref[2], z],
        "ra = 1 for 2.5": Lc.adjoint64(sx, sy, eta, s, ra=1.0),
        "inv_h = 126 for 63": Lc.adjoint64(sx, sy, eta, s, ih=126.0),
        "the 0.25 cross terms dropped": Lc.adjoint64(sx, sy, eta, s, cross=0.0),
        "the face viscosity from one node": Lc.adjoint64(sx, sy, eta, s, face="node"),
        "scaler of the wrong sample": Lc.adjoint64(sx, sy, eta, s.roll(1)),
    }


@pytest.mark.parametrize("H,W", [(5, 5), (9, 66)])
def test_adjoint_mutants_fail(H, W):
    """F2, the momentum mutants: fed as the kernel's output (gradient planes in the order u, v, p, T) to the comparison of part A."""
    c = Lc.adjoint_case(Lc.B, H, W)
    names = ("gu", "gv", "gp", "gT")
    assert Lc.check_planes(names, [Lc.stored(t) for t in c["ref"]], c["ref"], c["tol"])[0] == []
    for name, m in _adjoint_mutants(c).items():
        assert Lc.check_planes(names, [Lc.stored(t) for t in m], c["ref"], c["tol"])[0], name


def test_nonzero_ring_fails():
    d = Lc.inputs(Lc.B, 9, 66)
    r = Lc.Residual(d, 1e-6)
    good = (Lc.stored(r.sx), Lc.stored(r.sy), Lc.stored(r.eta), r.sums)
    assert Lc.check_residual(r, *good)[0] == []
    sx = good[0].clone()
    sx[:, 0, :] = r.c
    assert Lc.check_residual(r, sx, *good[1:])[0]
    assert Lc.check_residual(r, good[0], good[1], good[2], (r.sums[0] * 1.001, r.sums[1]))[0]


@pytest.mark.parametrize("name,kw,mut", [
    ("curl-type wall weights at x == 0", dict(p_pred=True, loss_type=2, ls=True, ld=True, l2=False, t_grad=1), dict(wall0=True)),
    ("border weight 11 on a 1-pixel frame", dict(p_pred=True, loss_type=1, ls=True, ld=False, l2=False, t_grad=1), dict(frame=1)),
    ("derivative normalisations swapped", dict(p_pred=True, loss_type=1, ls=False, ld=True, l2=False, t_grad=1), dict(swap_norm=True)),
])
def test_data_term_mutants_fail(name, kw, mut):
    d = Lc.inputs(Lc.B, 9, 66)
    ref, m = Lc.StokesGrad(d, **kw), Lc.StokesGrad(d, **kw, **mut)
    assert Lc.check_planes(Lc.PLANES, [Lc.stored(t) for t in ref.grad], ref.grad, ref.tol, ref.keep)[0] == []
    assert Lc.check_planes(Lc.PLANES, [Lc.stored(t) for t in m.grad], ref.grad, ref.tol, ref.keep)[0], name
    assert Lc.check_scalars(Lc.OUT_NAMES, m.out, ref.out, ref.out_tol)[0], name


def test_momentum_mutants_fail_in_the_one_launch_comparison():
    """Part C's comparison (lambda = 1, truth = prediction) rejects the dropped dP and the dropped buoyancy adjoint too."""
    d = Lc.inputs(Lc.B, 9, 66)
    truth = torch.stack([d["u"], d["v"], d["p"], d["T"]], 1)
    g = Lc.StokesGrad(d, truth=truth, p_pred=True, loss_type=0, ls=False, ld=False, l2=False, t_grad=1, lam=1.0)
    got = [Lc.stored(t) for t in g.grad]
    assert Lc.check_planes(Lc.PLANES, got, g.grad, g.tol, g.keep)[0] == []
    for j in (2, 3):
        m = list(got)
        m[j] = torch.zeros_like(m[j])
        assert Lc.check_planes(Lc.PLANES, m, g.grad, g.tol, g.keep)[0], Lc.PLANES[j]


def test_blocked_clip_gradient_fails():
    c = Lc.curl_case(23, 31)
    at = (c["t"] == Lc.T_LO) | (c["t"] == Lc.T_HI)
    assert bool(at.any()) and bool((c["gt_in"][at] == c["gt"][at]).all())
    m = torch.where(at, torch.zeros_like(c["gt"]), c["gt_in"])
    assert Lc.check_planes(["gt_in"], [c["gt_in"]], [c["gt_in"]], [0.0])[0] == []
    assert Lc.check_planes(["gt_in"], [m], [c["gt_in"]], [0.0])[0]


@pytest.mark.parametrize("H,W", [(29, 41), (70, 131), (5, 200)])
def test_existing_momentum_check_is_blind_to_the_small_parts(H, W):
    """F3: the comparison of test_hip_train.test_momentum_residual_matches_oracle (|g - ref| <= 1e-7 + 2e-3 |ref| on >= 99.5 % of
    the pixels, lambda = 1e-6), restated on its exact inputs, passes a gradient whose momentum part of gp, or of gT, is missing.
    Median share of the momentum term in the total gradient over the three shapes: p 3e-4 to 5e-4, T 4e-6 to 7e-6 (u, v: 0.3 to
    0.9); at every pixel of both planes the whole momentum contribution is below that tolerance."""
    Bn, lam = 2, 1e-6
    u = fields.smooth_field(Bn, H, W, 301, noise=0.01)
    v = fields.smooth_field(Bn, H, W, 302, noise=0.01)
    p = fields.smooth_field(Bn, H, W, 303, amp=0.5)
    T = fields.temperature_field(Bn, H, W, 304)
    uvp = np.stack([fields.smooth_field(Bn, H, W, 305), fields.smooth_field(Bn, H, W, 306), fields.smooth_field(Bn, H, W, 307, amp=0.5),
                    fields.temperature_field(Bn, H, W, 308)], 1)
    paras = fields.sim_parameters(Bn, 5)
    paras[:, 1] = 10.0 ** np.array([2.0, 3.0])
    scaler, yc = np.array([30.0, 80.0]), np.broadcast_to(np.linspace(0, 1, H)[:, None], (H, W)).copy()
    mom = dict(lambda_mom=lam, yc=torch.from_numpy(yc), paras=torch.from_numpy(paras), scaler=torch.from_numpy(scaler))
    grads = []
    for m in (mom, None):
        lv = [torch.from_numpy(a).to(f64).requires_grad_(True) for a in (u, v, p, T)]
        O.get_loss_unet(tuple(lv), torch.from_numpy(uvp).to(f64), p_pred=True, loss_type="mass", momentum=m)[0].backward()
        grads.append([t.grad for t in lv])
    full, without = grads
    for i in (2, 3):                                   # p, T
        part = full[i] - without[i]
        tol = 1e-7 + 2e-3 * full[i].abs()
        assert bool((part.abs() <= tol).all())
        bad = (without[i] - full[i]).abs() > tol       # the mutant's plane through the existing comparison
        assert float(bad.double().mean()) < 5e-3
        share = float((part.abs() / full[i].abs().clamp_min(1e-300)).median())
        print(f"\n{H}x{W} plane {'uvpT'[i]}: median share of the momentum term {share:.2e}")
        assert share < 1e-3
    for i in (0, 1):                                   # on u and v the term is visible
        assert float(((full[i] - without[i]).abs() / full[i].abs().clamp_min(1e-300)).median()) > 0.1

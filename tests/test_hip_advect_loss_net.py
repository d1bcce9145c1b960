"""GPU: the advection loss through the public layers.  StokesLoss.evaluate(advect=...) on a given network output against the
f64 reference of tests/advect_loss_ref.py (both sides see the same predictions, so the upwind masks cannot differ) for every
head of the FluidNet family; Trainer(model_AD=ADNet(...)) eager against captured, the resident step against the hand-fed one,
the unchanged `-ad 0` path, the run state, load_train_objs and the command line.

Bounds.  The six scalars: the bounds of the FluidNet-branch test of tests/test_hip_train.py (atol 1e-6, rtol 2e-5: f32 outputs
of f64 sums of f32 partials); loss_T alone also within the derived bound of the kernel test.  The gradient: U = 2^-24.  A value of
a gradient PLANE (d loss / d u, d loss / d v) carries at most K_GRAD = 20 roundings (tests/loss_cases.py) relative to the
magnitudes of its terms, and the advection increment's read-modify-write one more relative to what the plane holds.  What a
plane holds is bounded by P = the reference's largest plane value + the largest divergence-sign term of a pixel, M_w = wc + wr
('curl': 1 / (N (H-2)) + 1 / (N (W-2))), wm ('mass') or 0 ('mae') -- added because the velocity of a curl head is
divergence-free: its D is exactly 0 in f64 and rounding noise of either sign in f32, so the device's planes hold +-M_w / 2
terms next to the walls that the reference's do not; they cancel through the head's adjoint (curl^T div^T = 0), but only to
the rounding of their own size.  An element of gy is a plane value ('mae', 'mass') or a_bound / 2 times at most 6 plane
values (the four taps of the curl adjoint, two more at an antisymmetric wall) with at most 7 more roundings:
K_NET = 20 + 1 + 7 = 28, tol = K_NET U (|ref| + S), S = P or 3 a_bound P.  Pixels that a kink rule of
tests/advect_loss_ref.py leaves out (evaluated on THIS output's velocities) are left out, with their 3 x 3 neighbours where a
head's adjoint spreads them.  (Measured on MI355X: the largest |error| / bound is 0.01 - 0.04 for every head.)"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import advect_loss_ref as A
import run_state_worker as Wk
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f64 = torch.float64
N, H, W = 3, 37, 66
A_BOUND = 4.0
K_NET = 28


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def _output(head, p_pred):
    """The network output y (numpy f64 holding f32) of a head on the seeded case, and (H, W) of its planes."""
    c = A.case(N, H, W)
    if head in ("mae", "mass"):
        return np.stack([c["up"], c["vp"]] + ([c["pp"]] if p_pred else []), 1)
    import fields
    g = 2 if head == "curl_valid" else 0
    psi = A.r32(fields.smooth_field(N, H + g, W + g, 77, amp=1.0, noise=0.02) * (2.0 / A_BOUND))
    return np.stack([psi] + ([c["pp"]] if p_pred else []), 1)


def _velocities(head, ty, p_pred):
    """(u, v, p) [N,H,W] of the reference from the output tensor ty."""
    if head in ("mae", "mass"):
        return ty[:, 0], ty[:, 1], ty[:, 2] if p_pred else None
    if head == "curl":
        cu, cv = O.curl_head(ty[:, 0:1] * A_BOUND)
        return cu[:, 0], cv[:, 0], ty[:, 1] if p_pred else None
    a = A_BOUND * ty[:, 0]                                    # FluidNet: plain centred differences of the grown field
    return 0.5 * (a[:, 2:, 1:-1] - a[:, :-2, 1:-1]), -0.5 * (a[:, 1:-1, 2:] - a[:, 1:-1, :-2]), None


CONFIGS = [(h, p, "l1", False, False) for h in ("mae", "mass", "curl") for p in (False, True)] + [
    ("curl_valid", False, "l1", False, False), ("mass", True, "l2", False, False), ("curl", False, "l2", False, False),
    ("mae", True, "l1", True, True), ("curl", True, "l1", True, True), ("curl_valid", False, "l1", True, True)]


@pytest.mark.parametrize("cn", [A.CN_REF, A.CN_ADV])
@pytest.mark.parametrize("head,p_pred,norm,ls,ld", CONFIGS)
def test_evaluate_against_the_reference(head, p_pred, norm, ls, ld, cn):
    from pbml_mantle_convection_amd.losses import StokesLoss
    c = A.case(N, H, W)
    loss_type = "curl" if head == "curl_valid" else head
    y = _output(head, p_pred)
    ct = 3 if p_pred else 2
    Ls = StokesLoss(p_pred, loss_type, ls, ld, norm=norm, a_bound=A_BOUND, has_T=False, curl_valid=head == "curl_valid",
                    advect_cn=cn)
    out8, gy = Ls.evaluate(dev(y), dev(c["uvp"][:, :ct]), advect=(dev(c["x"]), dev(c["s"])))
    torch.cuda.synchronize()
    dt = Ls.adv_dt.cpu().numpy()
    assert dt.tobytes() == A.dt32(c, cn).tobytes()                                  # the truth's step: the head does not matter
    ty = torch.from_numpy(y).to(f64).requires_grad_(True)
    u, v, p = _velocities(head, ty, p_pred)
    u.retain_grad()
    v.retain_grad()
    ref = A.full_loss(c, dt, (u, v, p), p_pred=p_pred, loss_type=loss_type, loss_scale=ls, loss_derivative=ld, norm=norm)
    ref[0].backward()
    got, want = out8[:6].double().cpu().numpy(), np.array([float(r.detach()) for r in ref])
    print(f"\n{head} p_pred={p_pred} {norm} ls={ls} ld={ld} cn={cn}: out6 {got} ref {want}")
    assert (np.abs(got - want) <= 1e-6 + 2e-5 * np.abs(want)).all(), (got, want)
    assert float(out8[6]) == 0.0 and float(out8[7]) == 0.0 and want[4] > 0
    cc = dict(c, up=u.detach().numpy(), vp=v.detach().numpy())
    d = A.direct(cc, dt, norm, p_pred)
    assert abs(got[4] * N * H * W - d["sum"]) <= d["sum_tol"] + A.U * d["sum"], (got[4] * N * H * W, d["sum"], d["sum_tol"])
    ku, kv, share = A.keep_masks(A.direct(cc, dt, "l1", p_pred))
    assert share <= A.MAX_SHARE
    keep = torch.from_numpy(ku & kv)
    ring = torch.ones((N, H, W), dtype=torch.bool)
    ring[:, 1:-1, 1:-1] = False
    keep = keep | ring                                                              # (the ring carries no advection term)
    g = 2 if head == "curl_valid" else 0
    if head in ("curl", "curl_valid"):                                              # a left-out pixel reaches its neighbours' psi
        bad = F.max_pool2d(F.pad((~keep).double().unsqueeze(1), (g // 2,) * 4), 3, 1, 1)[:, 0] > 0
        keep0 = ~bad
    else:
        keep0 = keep
    gref = ty.grad
    m_w = {"mae": 0.0, "mass": 1.0 / (N * (H - 2) * (W - 2)), "curl": 1.0 / (N * (H - 2)) + 1.0 / (N * (W - 2))}[loss_type]
    P = max(float(u.grad.abs().max()), float(v.grad.abs().max())) + m_w
    S = P if head in ("mae", "mass") else 3.0 * A_BOUND * P
    tol = K_NET * A.U * (gref.abs() + S)
    err = (gy.double().cpu() - gref).abs()
    mask = torch.ones_like(gref, dtype=torch.bool)
    mask[:, 0] = keep0
    if head in ("mae", "mass"):
        mask[:, 1] = keep0
    worst = float((err / tol)[mask].max())
    print(f"  gy: largest |error| / bound {worst:.3f} over {int(mask.sum())} of {mask.numel()} elements, max |ref| {float(gref.abs().max()):.3e}, "
          f"S {S:.3e}")
    assert worst <= 1.0
    # the term is there: without it the loss and the gradient are others
    Ls0 = StokesLoss(p_pred, loss_type, ls, ld, norm=norm, a_bound=A_BOUND, has_T=False, curl_valid=head == "curl_valid")
    out0, gy0 = Ls0.evaluate(dev(y), dev(c["uvp"][:, :ct]))
    assert float(out0[4]) == 0.0 and not torch.equal(gy0, gy)
    assert torch.equal(out0[1:4], out8[1:4]) and torch.equal(out0[5], out8[5])     # the other scalars do not see the term


def test_argument_checks():
    from pbml_mantle_convection_amd.losses import StokesLoss
    with pytest.raises(ValueError, match="has_T"):
        StokesLoss(True, "mass", advect_cn=2e4)
    c = A.case(N, H, W)
    y, uvp, x, s = dev(_output("mass", True)), dev(c["uvp"]), dev(c["x"]), dev(c["s"])
    with pytest.raises(ValueError, match="advect"):
        StokesLoss(True, "mass", has_T=False, advect_cn=2e4).evaluate(y, uvp)
    with pytest.raises(ValueError, match="advect"):
        StokesLoss(True, "mass", has_T=False).evaluate(y, uvp, advect=(x, s))
    with pytest.raises(ValueError, match=">= 7"):
        StokesLoss(True, "mass", has_T=False, advect_cn=2e4).evaluate(y, uvp, advect=(x[:, :6].contiguous(), s))


# ------------------------------------------------------------------------------------------------------------------- Trainer
TH, TW, TB = 16, 40, 3


def _batch(p_pred):
    """(gVTp, uvp, scaler) on the device at 16 x 40, batch 3: the seeded case with the wall coordinates written into x (the
    network reads every channel)."""
    c = A.case(TB, TH, TW)
    x = c["x"].copy()
    x[:, 0, :, 0], x[:, 0, :, -1], x[:, 1, 0, :], x[:, 1, -1, :] = 0.0, 1.0, 0.0, 0.25
    assert np.isfinite(x).all()
    return dev(x), dev(c["uvp"][:, :3 if p_pred else 2]), dev(c["s"])


def _model(net, seed=4):
    from pbml_mantle_convection_amd.multigpu import build_model
    torch.manual_seed(seed)
    if net == "newfluidnet":
        return build_model("newfluidnet", 2, 7, 8, 3, torch.device(DEV), "gelu", "zeros", "mass", True, 1, 3, p_pred=True)
    return build_model("fluidnet", 2, 7, 8, 1, torch.device(DEV), "gelu", "replicate", "curl", False, 1, 5, p_pred=False)


def _trainer(net, model_AD, use_graph=False, train=None, cv=None, seed=4, nn_dir="/tmp/", **kw):
    from pbml_mantle_convection_amd.multigpu import Trainer
    m = _model(net, seed)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=kw.pop("milestones", [100]), gamma=0.5)
    p_pred = net == "newfluidnet"
    return Trainer(m, model_AD, train, cv, None, None, opt, sch, 0, 1, nn_dir, p_pred=p_pred, network=net, loss_scale=True,
                   loss_type="mass" if p_pred else "curl", precision="fp32", use_graph=use_graph, drop_seed=0, **kw)


def _adnet(cn=2e4):
    from pbml_mantle_convection_amd.pytorch_networks_convae import ADNet
    return ADNet(device=0, CN_max=cn)


@pytest.mark.parametrize("net", ["newfluidnet", "fluidnet"])
def test_trainer_eager_and_captured_steps_are_bit_identical(net):
    gVTp, uvp, s = _batch(net == "newfluidnet")
    res = []
    for use_graph in (False, True):
        tr = _trainer(net, _adnet(), use_graph)
        assert tr.advect_cn == 2e4 and tr.loss.advect_cn == 2e4
        outs = [tr.train_step(gVTp, uvp, scaler=s).clone() for _ in range(2)]
        torch.cuda.synchronize()
        res.append((*outs, tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
        assert all(float(o[4]) > 0 and bool(torch.isfinite(o).all()) for o in outs)
        with torch.no_grad():
            ev = tr.eval_step(gVTp, uvp, scaler=s)
        assert float(ev[4]) > 0
    for a, b in zip(*res):
        assert torch.equal(a, b), float((a - b).abs().max())
    # the autograd-visible form gives the same loss as the fused one's first step, on the same weights
    tr = _trainer(net, _adnet())
    out = tr.get_loss(gVTp, uvp, s)
    out[0].backward()
    assert torch.equal(torch.stack([o.detach().reshape(()) for o in out]), res[0][0][:6])
    with pytest.raises(ValueError, match="scaler"):
        tr.train_step(gVTp, uvp)


@pytest.mark.parametrize("net", ["newfluidnet", "fluidnet"])
def test_without_model_ad_the_step_is_the_one_without_the_term(net):
    """model_AD = None: out8 and the flat gradient are bit-identical to those of a loss object built without advect_cn."""
    from pbml_mantle_convection_amd.losses import StokesLoss
    gVTp, uvp, s = _batch(net == "newfluidnet")
    a, b = _trainer(net, None), _trainer(net, None)
    assert a.advect_cn is None and a.loss.advect_cn is None and a.model_AD is None
    p_pred = net == "newfluidnet"
    b.loss = StokesLoss(p_pred, "mass" if p_pred else "curl", True, False, a_bound=getattr(b.model_uvp, "a_bound", 10.0), has_T=False,
                        curl_valid=not p_pred)
    oa = a._fwd_bwd(gVTp, uvp, None, None, s).clone()
    ob = b._fwd_bwd(gVTp, uvp, None, None, None).clone()
    assert torch.equal(oa, ob) and float(oa[4]) == 0.0 and torch.equal(a.flat.grad, b.flat.grad) and bool(a.flat.grad.any())
    c = _trainer(net, _adnet())
    oc = c._fwd_bwd(gVTp, uvp, None, None, s)
    assert float(oc[4]) > 0 and not torch.equal(c.flat.grad, a.flat.grad)
    assert torch.equal(oc[1:4], oa[1:4]) and torch.equal(oc[5], oa[5])           # the other scalars do not see the term


def test_unet_accepts_and_ignores_model_ad(capfd):
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import Unet
    torch.manual_seed(0)
    m = Unet(2, 10, 8, 3, torch.device(DEV), "gelu", "reflect", "mass", use_symm=True, repeats=1, f=3, p_pred=False)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.5)
    tr = Trainer(m, _adnet(), None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=False, network="unet", loss_type="mass")
    assert tr.advect_cn is None and tr.loss.advect_cn is None
    assert "does not use model_AD" in capfd.readouterr().err
    with pytest.raises(TypeError, match="ADNet"):
        _trainer("newfluidnet", object())


def test_resident_step_equals_the_host_batch(golden, tmp_path):
    """A: ResidentLoaders, captured (the replay assembles x, truth and scaler).  B: eager, fed with `assemble` of the same rows.
    Losses, parameters and moments stay bit-identical; the cv step too."""
    from pbml_mantle_convection_amd.datasetio import NewADDataset, ResidentLoader, ResidentNewADDataset
    Wk.write_tree(golden("g18_newad_dataset"), str(tmp_path))
    kw = dict(scale=True, load=False, p_pred=True, debug=False, noise=0.0)
    dss = [NewADDataset(str(tmp_path), an, is_init=init, **kw) for an in ("train", "cv") for init in (False, True)]
    tr_res, tr_init, cv_res, cv_init = (ResidentNewADDataset(d, DEV, is_init=bool(k % 2)) for k, d in enumerate(dss))
    loaders = [ResidentLoader(tr_res, tr_init, batch_size=4, small_batch=2, seed=3),
               ResidentLoader(cv_res, cv_init, batch_size=4, small_batch=2, seed=3)]
    stores = [(tr_res, tr_init), (cv_res, cv_init)]
    Atr = _trainer("newfluidnet", _adnet(), True, loaders[0], loaders[1])
    Btr = _trainer("newfluidnet", _adnet(), False)
    for which, ld in enumerate(loaders):
        ld.start_epoch(0)
        for step in range(len(ld)):
            row = ld.table_host[step].tolist()
            parts = [(stores[which][0].assemble([e]) if e >= 0 else stores[which][1].assemble([-e - 1])) for e in row]
            x, y, _, sc = (torch.cat([p[k] for p in parts]) for k in range(4))
            if which == 0:
                la, lb = Atr.resident_step(ld, True).clone(), Btr.train_step(x, y, scaler=sc).clone()
                torch.cuda.synchronize()
                assert torch.equal(Atr.flat.param, Btr.flat.param) and torch.equal(Atr.exp_avg_sq, Btr.exp_avg_sq), step
            else:
                with torch.no_grad():
                    la, lb = Atr.resident_step(ld, False).clone(), Btr.eval_step(x, y, scaler=sc).clone()
            assert torch.equal(la, lb) and float(la[4]) > 0 and bool(torch.isfinite(la).all()), (which, step, la, lb)
    assert Atr._graph is not None and Atr.input_buffers()["scaler"].data_ptr() == loaders[0].out["scaler"].data_ptr()


def _run(nn_dir, seed, epochs, model_AD, epoch=0, state=None, **kw):
    gVTp, uvp, s = _batch(True)
    z = torch.zeros(TB)
    items = [(gVTp.cpu(), uvp.cpu(), z, s.cpu()), (gVTp.flip(0).cpu(), uvp.flip(0).cpu(), z, s.flip(0).cpu())]
    os.makedirs(nn_dir, exist_ok=True)
    tr = _trainer("newfluidnet", model_AD, True, Wk.Batches(items), Wk.Batches(items[:1]), seed=seed, nn_dir=str(nn_dir) + "/",
                  milestones=Wk.MILESTONES, epoch=epoch, **kw)
    if state is not None:
        tr.load_state(state)
    tr.train(epochs)
    return tr


def test_run_state_records_the_term_and_resumes_bit_for_bit(tmp_path):
    from pbml_mantle_convection_amd.multigpu import STATE_FILE, read_state_file
    with open(tmp_path / "x", "w"):
        pass
    for d in ("A", "B"):
        os.makedirs(tmp_path / d)
        with open(tmp_path / d / "fluidnet_uvpT.txt", "w") as fw:
            fw.write("Epoch, train loss, val loss, learning rate \n")
    a = Wk.result(_run(tmp_path / "A", 3, Wk.EPOCHS, _adnet()))
    _run(tmp_path / "B", 3, Wk.STOP, _adnet(), save_state=True)
    path = str(tmp_path / "B" / STATE_FILE)
    h = read_state_file(path)["header"]
    assert h["advect"] is True and h["CN_max"] == 2e4
    b = Wk.result(_run(tmp_path / "B", 77, Wk.EPOCHS, _adnet(), epoch=Wk.STOP, state=path))
    a["log"], b["log"] = a["log"][1:], b["log"][1:]                                 # (the header line of the text log)
    assert Wk.same(a, b) == []
    for other in (_adnet(0.1), None):
        with pytest.raises(ValueError, match="CN_max"):
            _run(tmp_path / "B", 77, Wk.EPOCHS, other, epoch=Wk.STOP, state=path)
    # a state written without the term does not continue a run with it
    _run(tmp_path / "A", 3, 1, None, save_state=True)
    assert read_state_file(str(tmp_path / "A" / STATE_FILE))["header"]["advect"] is False
    with pytest.raises(ValueError, match="CN_max"):
        _run(tmp_path / "A", 77, 2, _adnet(), epoch=1, state=str(tmp_path / "A" / STATE_FILE))


def test_load_train_objs_and_the_command_line(tmp_path, monkeypatch):
    import torch.distributed as dist
    from pbml_mantle_convection_amd import multigpu as G
    from pbml_mantle_convection_amd.pytorch_networks_convae import ADNet
    objs = G.load_train_objs(0, 1, str(tmp_path) + "/", "", 2, 7, 8, 3, "gelu", "zeros", "mass", True, 1, 3, [100], {}, {}, {}, {},
                             p_pred=True, advect=True, network="newfluidnet", synthetic=dict(n=4, H=TH, W=TW))
    assert isinstance(objs[3], ADNet) and objs[3].CN_max == 2e4
    assert G.load_train_objs(0, 1, str(tmp_path) + "/", "", 2, 7, 8, 3, "gelu", "zeros", "mass", True, 1, 3, [100], {}, {}, {}, {},
                             p_pred=True, advect=False, network="newfluidnet", synthetic=dict(n=4, H=TH, W=TW))[3] is None
    a = G.build_arg_parser().parse_args(["-ad", "1"])
    assert a.advect == 1 and a.ad_cn == 2e4 and G.build_arg_parser().parse_args(["--ad_cn", "0.5"]).ad_cn == 0.5
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    logs = {}
    for ad in ("0", "1"):
        try:
            G.cli(["-net", "newfluidnet", "-l", "2", "-f", "8", "-r", "1", "-k", "3", "-p", "zeros", "-lt", "mass", "-pp", "1", "-s", "1",
                   "-ab", "10", "-b", "2", "-deb", "1", "-ad", ad, "--synthetic", "4", str(TH), str(TW), "--epochs", "1", "--nn_root",
                   str(tmp_path / ("nn" + ad)), "--precision", "fp32", "--use_graph", "1"])
        finally:
            if dist.is_initialized():
                dist.destroy_process_group()
        runs = os.listdir(tmp_path / ("nn" + ad))
        assert len(runs) == 1 and ("_adTrue_" if ad == "1" else "_adFalse_") in runs[0]
        line = open(tmp_path / ("nn" + ad) / runs[0] / "fluidnet_uvpT.txt").read().strip().split("\n")[-1]
        logs[ad] = [float(v) for v in line.split("[")[1].split("]")[0].split(",")]
    # the log's train losses are (u, v, p, T, mass): the T column is the term's
    assert logs["0"][3] == 0.0 and logs["1"][3] > 0.0 and np.isfinite(logs["1"]).all()

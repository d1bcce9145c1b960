"""FluidNet (`-net fluidnet`, the CLI default) on the HIP path: the grown-field curl kernels against a numpy stencil, the
network's forward and every parameter gradient against the reference (golden g22), the trainer's loss and gradients (eager
and captured), the 16-bit modes against fp32, graph / eager bit identity and the CLI end to end."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fields

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype).to(DEV)


def assert_close(a, b, atol, rtol=1e-4, what=""):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e} (tol {atol}+{rtol}*|ref|), MAE {err.mean():.3e}"


def curl_np(a, ab):
    """u, v on H x W from an (H+2) x (W+2) streamfunction (reference pytorch_networks_convae.py:1681-1697)."""
    a = ab * a.astype(np.float64)
    return 0.5 * (a[..., 2:, 1:-1] - a[..., :-2, 1:-1]), -0.5 * (a[..., 1:-1, 2:] - a[..., 1:-1, :-2])


def curl_adj_np(gu, gv, ab):
    B, H, W = gu.shape
    ga = np.zeros((B, H + 2, W + 2))
    ga[:, 2:, 1:-1] += 0.5 * ab * gu
    ga[:, :-2, 1:-1] -= 0.5 * ab * gu
    ga[:, 1:-1, 2:] -= 0.5 * ab * gv
    ga[:, 1:-1, :-2] += 0.5 * ab * gv
    return ga


@pytest.mark.parametrize("B,H,W", [(3, 9, 13), (2, 128, 506), (1, 1, 1), (2, 31, 70)])
def test_curl_valid_kernels_vs_stencil(B, H, W):
    """Forward elementwise, backward elementwise and as the adjoint, on the streamfunction channel of a 3-channel tensor
    (batch stride larger than the plane); the backward writes every pixel of channel 0 and nothing else."""
    from pbml_mantle_convection_amd import _lib as L
    L.load()
    rng = np.random.RandomState(H * 1000 + W)
    ab = 10.0
    y = rng.standard_normal((B, 3, H + 2, W + 2)).astype(np.float32)
    yd = dev(y)
    u = torch.empty((B, H, W), device=DEV)
    v = torch.empty_like(u)
    plane = 3 * (H + 2) * (W + 2)
    L.call("mc_curl_valid_fwd", L.ptr(yd), B, H, W, plane, ab, L.ptr(u), L.ptr(v), L.stream())
    ru, rv = curl_np(y[:, 0], ab)
    assert_close(u, ru, atol=1e-5, rtol=1e-6, what="u")
    assert_close(v, rv, atol=1e-5, rtol=1e-6, what="v")
    gu = rng.standard_normal((B, H, W)).astype(np.float32)
    gv = rng.standard_normal((B, H, W)).astype(np.float32)
    gud, gvd = dev(gu), dev(gv)
    ga = torch.full((B, 3, H + 2, W + 2), float("nan"), device=DEV)
    ga[:, 1:] = 7.0
    L.call("mc_curl_valid_bwd", L.ptr(gud), L.ptr(gvd), B, H, W, ab, L.ptr(ga), plane, L.stream())
    torch.cuda.synchronize()
    assert bool((ga[:, 1:] == 7.0).all()), "wrote outside channel 0"
    assert bool(torch.isfinite(ga[:, 0]).all()), "left pixels of channel 0 unwritten"
    ref = curl_adj_np(gu, gv, ab)
    assert_close(ga[:, 0], ref, atol=1e-5, rtol=1e-6, what="ga")
    lhs = float((u.double() * gud.double()).sum() + (v.double() * gvd.double()).sum())
    rhs = float((yd[:, 0].double() * ga[:, 0].double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1e-30) + 1e-6, (lhs, rhs)
    # launch twice: the gather is bit-reproducible
    ga2 = torch.empty((B, 3, H + 2, W + 2), device=DEV)
    L.call("mc_curl_valid_bwd", L.ptr(gud), L.ptr(gvd), B, H, W, ab, L.ptr(ga2), plane, L.stream())
    assert torch.equal(ga[:, 0], ga2[:, 0])


def _model(g, r_p="learned"):
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm = [int(v) for v in g["cfg"][:8]]
    m = FluidNet(levels, c_i, c_h, c_o, torch.device(DEV), "gelu", r_p, "curl", use_symm=bool(symm),
                 a_bound=float(g["a_bound"]) if "a_bound" in g.files else 10.0, repeats=repeats, f=f, p_pred=bool(p_pred))
    sd = {n[3:]: torch.from_numpy(g[n]).float() for n in g.files if n.startswith("sd/")}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("tag,seed", [("learned", 220), ("replicate", 225)])
def test_fluidnet_vs_golden(golden, tag, seed):
    """fp32 forward (u, v) and every parameter gradient against the reference FluidNet (learned padding: conv.1 with
    bc_x = bc_y = 2; replicate: the constructor's padding-2 conv.1)."""
    g = golden(f"g22_fluidnet_{tag}")
    m = _model(g, str(g["r_p"]))
    x = dev(fields.unet_input(1, 128, 506, seed + 2, c_i=7))
    with torch.no_grad():
        assert tuple(m.features(x).shape) == (1, 1, 130, 508)
    u, v, p = m(x)
    assert p is None and tuple(u.shape) == (1, 128, 506) and tuple(v.shape) == (1, 128, 506)
    loss = 0.0
    for i, (n, o) in enumerate((("u", u), ("v", v))):
        ref = g["out/" + n]
        assert_close(fields.strided_sample(o.detach().cpu().numpy(), 20001), ref,
                     atol=3e-5 * max(1.0, float(np.abs(ref).max())), rtol=2e-4, what="out " + n)
        loss = loss + (o * dev(fields.smooth_field(1, 128, 506, seed + 3 + i).astype(np.float32))).sum()
    loss.backward()
    for n, prm in m.named_parameters():
        ref = g["grad/" + n]
        if float(np.abs(ref).max()) < 1e-6:
            continue                                    # null directions (the last layer's shared bias under the zero-mean)
        assert_close(prm.grad, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=3e-3, what="grad " + n)


def _trainer(m, prec="fp32", use_graph=False, lr=1e-3):
    from pbml_mantle_convection_amd.multigpu import Trainer
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1000], gamma=0.5)
    return Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=False, network="fluidnet",
                   loss_scale=True, loss_derivative=True, loss_type="curl", precision=prec, use_graph=use_graph)


def _batch():
    B, H, W = 2, 128, 506
    gVTp = dev(fields.unet_input(B, H, W, 2230, c_i=7))
    uvp = dev(np.stack([fields.smooth_field(B, H, W, 2231), fields.smooth_field(B, H, W, 2232)], 1))
    return gVTp, uvp


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_trainer_loss_and_gradients_vs_golden(golden, mode):
    """Trainer.get_loss of the reference (FluidNet branch, loss_scale = loss_derivative = 1): the six losses and every
    parameter gradient, through the autograd path (eager) and through one HIP-graph-captured training step."""
    g = golden("g22_fluidnet_get_loss")
    m = _model(golden("g22_fluidnet_learned"))
    gVTp, uvp = _batch()
    if mode == "eager":
        tr = _trainer(m)
        out = tr.get_loss(gVTp, uvp, None)
        out[0].backward()
        got = torch.stack([o.detach().reshape(()) for o in out])
        grads = {n: p.grad for n, p in m.named_parameters()}
    else:
        tr = _trainer(m, use_graph=True)
        got = tr.train_step(gVTp, uvp)[:6].clone()
        torch.cuda.synchronize()
        grads = tr.flat.views(tr.flat.grad)
    assert_close(got, g["losses"], atol=1e-6, rtol=1e-4, what="losses")
    for n, gr in grads.items():
        ref = g["grad/" + n]
        if float(np.abs(ref).max()) < 1e-6:
            continue
        assert_close(gr, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=3e-3, what="grad " + n)


def _step_state(golden, prec):
    m = _model(golden("g22_fluidnet_learned"))
    tr = _trainer(m, prec)
    gVTp, uvp = _batch()
    out = tr.get_loss(gVTp, uvp, None)
    out[0].backward()
    flat = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).double()
    return float(out[0].detach()), flat


# relative loss gap / flat-gradient rel-L2 gap to fp32, about 1.5 x what MI355X measured (bf16: 3.0e-2 / 1.9e-2, mixed:
# 1.6e-3 / 3.1e-3).  The learned-padding head stores its output in the 16-bit type in these modes; the curl
# of that output, scaled by a_bound = 10 and by the loss's boundary weights, is what the loss sees.
_GAP_BOUNDS = {"bf16": (4.5e-2, 3e-2), "mixed": (2.5e-3, 5e-3)}


@pytest.mark.parametrize("prec", ["bf16", "mixed"])
def test_16bit_modes_near_fp32(golden, prec):
    l32, g32 = _step_state(golden, "fp32")
    l16, g16 = _step_state(golden, prec)
    assert np.isfinite(l16) and bool(torch.isfinite(g16).all())
    dl = abs(l16 - l32) / abs(l32)
    dg = float((g16 - g32).norm() / g32.norm())
    print(f"{prec}: loss {l16:.6f} vs fp32 {l32:.6f} (rel {dl:.2e}), gradient rel-L2 {dg:.2e}")
    bl, bg = _GAP_BOUNDS[prec]
    assert dl < bl and dg < bg, (dl, dg)


def test_captured_steps_bit_identical_to_eager(golden):
    """Two HIP-graph-captured training steps leave the same parameters, Adam moments and losses as two eager ones."""
    gVTp, uvp = _batch()
    res = []
    for use_graph in (False, True):
        tr = _trainer(_model(golden("g22_fluidnet_learned")), use_graph=use_graph)
        outs = [tr.train_step(gVTp, uvp).clone() for _ in range(2)]
        torch.cuda.synchronize()
        res.append((*outs, tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("extra", [["-p", "learned"], ["--use_graph", "1"]])
def test_cli_end_to_end(tmp_path, extra):
    """`-net fluidnet` with the run list's flags on synthetic data in a child process on one device (learned padding eager;
    the default -p replicate captured): exits 0 and writes the reference-named checkpoint, which loads with strict=True."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet
    cmd = [sys.executable, "-m", "pbml_mantle_convection_amd.train", "-net", "fluidnet", "-l", "2", "-f", "8", "-r", "1", "-k", "5",
           "-b", "2", "-s", "0", "-ab", "10", "--synthetic", "4", "128", "506", "--epochs", "1", "-gpu", "0",
           "--nn_root", str(tmp_path) + "/"] + extra
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ck = glob.glob(str(tmp_path / "*" / "0_fluidnet_uvp.pt"))
    assert len(ck) == 1, os.listdir(tmp_path)
    sd = torch.load(ck[0], map_location="cpu", weights_only=True)
    r_p = "learned" if "learned" in extra else "replicate"
    m = FluidNet(2, 7, 8, 1, None, "gelu", r_p, "curl", use_symm=False, a_bound=10, repeats=1, f=5, p_pred=False)
    m.load_state_dict(sd, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())

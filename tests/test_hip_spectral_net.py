"""Spectral layers on the HIP path at the layer and network level: the stand-alone modules, NewFluidNet / FluidNet with
spectral_conv=True against the reference's f64 (golden g24) in all three precisions, two training steps against the
reference's (which pins Adam on the complex parameters), captured replay against eager launches, run-to-run bit identity,
and the CLI's -spectral 1."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fields
import spectral_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype).to(DEV)


def npy(t):
    t = t.detach().cpu()
    return t.to(torch.complex128).numpy() if t.is_complex() else t.double().numpy()


def assert_close(a, b, atol, rtol, what=""):
    a = npy(a) if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    assert (err <= atol + rtol * np.abs(b)).all(), f"{what}: max err {err.max():.3e} (ref max {np.abs(b).max():.3e})"


def grad_gate(got, ref, what):
    """The project's fp32 gate for a gradient tensor: rtol 2e-3 on a floor of 3e-4 of the tensor's scale."""
    assert_close(got, ref, atol=3e-4 * max(1.0, float(np.abs(ref).max())), rtol=2e-3, what=what)


def load_sd(m, g, prefix="sd/"):
    sd = {n[len(prefix):]: torch.from_numpy(g[n]) for n in g.files if n.startswith(prefix)}
    sd = {n: v.to(torch.complex64) if v.is_complex() else v.float() for n, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


# ------------------------------------------------------------------------------------------------ stand-alone modules
@pytest.mark.parametrize("tag", ["a", "b"])
def test_spectral_fluid_layer_vs_golden(golden, tag):
    """fp32 against the reference's SpectralFluidLayer: output within 2e-5 of its largest entry, dx and every parameter gradient
    at the gradient gate."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import SpectralFluidLayer
    g = golden("g24_spectral_layer")
    c_i, c_o, H, W = [int(v) for v in g[f"{tag}/meta"]]
    m = load_sd(SpectralFluidLayer(c_i, c_o, str(g[f"{tag}/act"]), "zeros", True, 1, f=5), g, f"{tag}/sd/")
    x = dev(g[f"{tag}/x"]).requires_grad_(True)
    y = m(x)
    ref = g[f"{tag}/y"]
    err = float(np.abs(npy(y) - ref).max())
    print(f"layer {tag}: output err {err:.3e} = {err / np.abs(ref).max():.2e} of max|ref|")
    assert err <= 2e-5 * np.abs(ref).max()
    (y * dev(g[f"{tag}/ct"])).sum().backward()
    grad_gate(x.grad, g[f"{tag}/dx"], "dx")
    for n, p in m.named_parameters():
        assert p.grad.dtype == p.dtype
        grad_gate(p.grad, g[f"{tag}/grad/{n}"], "grad " + n)


def test_spectral_conv2d_vs_restatement():
    """SpectralConv2d alone (no GroupNorm) against tests/spectral_ref.py, forward, dx and both weight gradients."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import SpectralConv2d
    torch.manual_seed(5)
    m = SpectralConv2d(5, 7, 12, 12).to(DEV)
    with torch.no_grad():
        for p in m.parameters():                      # (the init is non-negative: centre it so that signs matter)
            p.sub_(complex(0.5, 0.5) * m.scale)
    x = R.draw((2, 5, 9, 11), 31)
    dy = R.draw((2, 7, 9, 11), 32)
    w1, w2 = npy(m.weights1), npy(m.weights2)
    xd = dev(x).requires_grad_(True)
    y = m(xd)
    ref = R.conv_fwd(x, w1, w2)
    assert float(np.abs(npy(y) - ref).max()) <= 2e-5 * np.abs(ref).max()
    (y * dev(dy)).sum().backward()
    dx, d1, d2 = R.conv_bwd(x, w1, w2, dy)
    grad_gate(xd.grad, dx, "dx")
    grad_gate(m.weights1.grad, d1, "dweights1")
    grad_gate(m.weights2.grad, d2, "dweights2")


# measured on MI355X: 3.7e-7 of max|ref|; the bound is 1.5 x that.  2e-5 would be the fp32 output gate: a value
# above it means the summation order is wrong.
LARGE_LAYER_BOUND = 1.5 * 3.7e-7


def test_large_layer_summation_order():
    """One 16 -> 16 layer at 506 x 512 (32 slots of 32 rows x 256 columns per sample), fp32, against the f64 restatement."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import SpectralFluidLayer
    torch.manual_seed(6)
    m = SpectralFluidLayer(16, 16, "gelu")
    with torch.no_grad():
        for p in m.layers[0].parameters():
            p.sub_(complex(0.5, 0.5) * m.layers[0].scale)
    x = R.draw((1, 16, 506, 512), 41)
    x += fields.smooth_field(16, 506, 512, 42, amp=1.0)[None]      # (low modes above the noise floor, as a real field has)
    x = x.astype(np.float32).astype(np.float64)
    p64 = [p.detach().to(torch.complex128) if p.is_complex() else p.detach().double() for p in m.parameters()]
    ref = R.layer_torch(torch.from_numpy(x), *p64, "gelu").numpy()
    y = npy(m.to(DEV)(dev(x)))
    rel = float(np.abs(y - ref).max() / np.abs(ref).max())
    print(f"506 x 512 layer: output err {rel:.3e} of max|ref|")
    assert rel <= 2e-5, "the summation order is wrong"
    assert rel <= LARGE_LAYER_BOUND


# ------------------------------------------------------------------------------------------------ networks
def _newfluidnet(g, prec="fp32"):
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm = [int(v) for v in g["cfg"][:8]]
    m = NewFluidNet(levels, c_i, c_h, c_o, torch.device(DEV), "gelu", "zeros", "mae", use_symm=bool(symm), repeats=repeats, f=f,
                    p_pred=bool(p_pred), spectral_conv=True)
    return load_sd(m, g).set_precision(prec)


def _run_newfluidnet(g, prec):
    m = _newfluidnet(g, prec)
    outs = m(dev(fields.unet_input(1, 128, 506, 246, c_i=7)))
    loss, got = 0.0, {}
    for i, (n, o) in enumerate(zip("uvp", outs)):
        got[n] = fields.strided_sample(npy(o), 2003)
        g_ = torch.Generator().manual_seed(247 + i)          # tools/make_golden.py rnd(shape, 247 + i)
        ct = torch.randn(tuple(o.shape), generator=g_, dtype=torch.float32).to(DEV)
        loss = loss + (o * ct).sum()
    loss.backward()
    return m, got


def test_newfluidnet_spectral_vs_golden_fp32(golden):
    """Five levels, 128 x 506 ... 8 x 31 (the minimum a spectral layer takes): outputs and every parameter gradient."""
    g = golden("g24_newfluidnet_spectral")
    m, got = _run_newfluidnet(g, "fp32")
    for n in "uvp":
        ref = g["out/" + n]
        err = float(np.abs(got[n] - ref).max())
        print(f"newfluidnet fp32 out {n}: err {err:.3e} = {err / np.abs(ref).max():.2e} of max|ref|")
        assert err <= 2e-5 * np.abs(ref).max(), n
    for n, p in m.named_parameters():
        ref = g["grad/" + n]
        if float(np.abs(ref).max()) < 1e-6:
            continue                                    # null direction (the last conv's bias under the zero-mean)
        grad_gate(p.grad, ref, "grad " + n)


def _rel_l2(m, got, g):
    o = np.concatenate([got[n] for n in "uvp"])
    r = np.concatenate([g["out/" + n] for n in "uvp"])
    gg = np.concatenate([npy(p.grad).reshape(-1) for _, p in m.named_parameters()])
    gr = np.concatenate([g["grad/" + n].reshape(-1) for n, _ in m.named_parameters()])
    return float(np.linalg.norm(o - r) / np.linalg.norm(r)), float(np.linalg.norm(gg - gr) / np.linalg.norm(gr))


# relative L2 of the sampled outputs / of the flat gradient against the reference's f64, 1.5 x what MI355X measured
# (bf16: 5.72e-3 / 5.73e-3, mixed: 6.97e-4 / 1.39e-2)
_L2_BOUNDS = {"bf16": (1.5 * 5.72e-3, 1.5 * 5.73e-3), "mixed": (1.5 * 6.97e-4, 1.5 * 1.394e-2)}


@pytest.mark.parametrize("prec", ["bf16", "mixed"])
def test_newfluidnet_spectral_16bit_vs_golden(golden, prec):
    g = golden("g24_newfluidnet_spectral")
    m, got = _run_newfluidnet(g, prec)
    do, dg = _rel_l2(m, got, g)
    print(f"newfluidnet {prec}: rel-L2 outputs {do:.3e}, flat gradient {dg:.3e}")
    assert np.isfinite(do) and np.isfinite(dg)
    assert do <= _L2_BOUNDS[prec][0] and dg <= _L2_BOUNDS[prec][1], (do, dg)


def test_fluidnet_spectral_learned_curl_vs_golden(golden):
    """FluidNet(r_p='learned', loss_type='curl', p_pred=False, spectral_conv=True): a spectral trunk under learned-padding
    heads and the grown-field curl head, fp32 forward and every parameter gradient."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet
    g = golden("g24_fluidnet_spectral")
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm = [int(v) for v in g["cfg"][:8]]
    m = load_sd(FluidNet(levels, c_i, c_h, c_o, torch.device(DEV), "gelu", "learned", "curl", use_symm=bool(symm),
                         a_bound=float(g["a_bound"]), repeats=repeats, f=f, p_pred=bool(p_pred), spectral_conv=True), g)
    u, v, p = m(dev(fields.unet_input(1, 128, 506, 253, c_i=7)))
    assert p is None
    loss = 0.0
    for i, (n, o) in enumerate((("u", u), ("v", v))):
        ref = g["out/" + n]
        err = float(np.abs(fields.strided_sample(npy(o), 2003) - ref).max())
        print(f"fluidnet fp32 out {n}: err {err:.3e} = {err / np.abs(ref).max():.2e} of max|ref|")
        assert err <= 2e-5 * np.abs(ref).max(), n
        loss = loss + (o * dev(fields.smooth_field(1, 128, 506, 254 + i).astype(np.float32))).sum()
    loss.backward()
    for n, prm in m.named_parameters():
        ref = g["grad/" + n]
        if float(np.abs(ref).max()) < 1e-6:
            continue
        grad_gate(prm.grad, ref, "grad " + n)


# ------------------------------------------------------------------------------------------------ training
def _trainer(g, prec="fp32", use_graph=False, prefix="sd0/"):
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm, ls, ld = [int(v) for v in g["cfg"]]
    m = NewFluidNet(levels, c_i, c_h, c_o, torch.device(DEV), "gelu", "zeros", "mae", use_symm=bool(symm), repeats=repeats, f=f,
                    p_pred=bool(p_pred), spectral_conv=True)
    m = load_sd(m, g, prefix)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.5)
    tr = Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=bool(p_pred), network="newfluidnet",
                 loss_scale=bool(ls), loss_derivative=bool(ld), loss_type="mae", precision=prec, use_graph=use_graph)
    return m, tr


def _batch(step):
    B, H, W = 2, 128, 506
    gVTp = dev(fields.unet_input(B, H, W, 2400 + step, c_i=7))
    uvp = dev(np.stack([fields.smooth_field(B, H, W, 2410 + step), fields.smooth_field(B, H, W, 2420 + step),
                        fields.smooth_field(B, H, W, 2430 + step, amp=0.5)], 1))
    return gVTp, uvp


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_training_steps_golden(golden, use_graph):
    """zero_grad -> get_loss -> backward -> Adam twice against the reference (f32 mode), eager and captured: the losses (rtol
    5e-5) and the updated parameters, complex ones included (the existing two-step gate: 1e-4 + 1e-4 |ref|).

    Null directions are left out, as in the Unet's two-step test: where the reference's first gradient is below 1e-9 the
    device's is rounding noise, which Adam normalises to a step of up to lr whatever its size.  There the last conv's bias is
    the one such tensor; in a spectral layer the null directions are single entries -- the weights of the modes an input
    channel does not contain (a constant channel has only its DC mode, a coordinate channel only one row or column of
    modes) -- so the threshold is applied per element."""
    g = golden("g24_train_newfluidnet_spectral")
    m, tr = _trainer(g, use_graph=use_graph)
    for step in range(2):
        vals = tr.train_step(*_batch(step))[:6].tolist()
        ref = g["losses"][step]
        print(f"step {step}: losses {vals}, worst relative error {np.abs((np.array(vals) - ref) / np.maximum(np.abs(ref), 1e-30)).max():.2e}")
        assert_close(np.array(vals), ref, atol=1e-6, rtol=5e-5, what=f"losses step {step}")
        if step == 0:                                  # (the flat gradient stays as the step left it)
            grad0 = {n: npy(v) for n, v in tr.flat.views(tr.flat.grad).items()}
    # the masked entries must be null directions on the device as well: there the gradient is conj(Xhat) G with Xhat pure
    # rounding noise, at most 161 * 2^-24 ~ 1e-5 of the channel's sum of absolute values, and G varies between modes by up
    # to two orders of magnitude -> below 1e-3 of the tensor's largest reference gradient; a kernel that leaks energy into
    # modes the input does not contain would put O(1) of that scale there
    for n, gd in grad0.items():
        ref = g["grad0/" + n]
        ref = np.stack([ref.real, ref.imag], -1) if np.iscomplexobj(ref) else ref
        dead = np.abs(ref) < 1e-9
        if dead.any() and np.abs(ref).max() >= 1e-9:
            leak = float(np.abs(gd[dead]).max() / np.abs(ref).max())
            print(f"null entries of {n}: {int(dead.sum())}, largest device gradient {leak:.2e} of max|ref|")
            assert leak <= 1e-3, n
    bad = []
    for n, p in m.named_parameters():
        live = np.abs(g["grad0/" + n]) >= 1e-9
        ref, got = g["sd2/" + n], npy(p)
        err = np.where(live, np.abs(got - ref), 0.0)
        over = err > 1e-4 + 1e-4 * np.abs(ref)
        print(f"param {n}: {int(live.sum())}/{live.size} live entries, max err {err.max():.2e}, over the gate {int(over.sum())}")
        if over.any():
            bad.append(n)
    assert not bad, bad


def _three_steps(g, prec, use_graph):
    m, tr = _trainer(g, prec, use_graph)
    outs = [tr.train_step(*_batch(s % 2)).clone() for s in range(3)]
    torch.cuda.synchronize()
    return (*outs, tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.flat.grad.clone())


def test_captured_replay_equals_eager(golden):
    g = golden("g24_train_newfluidnet_spectral")
    for a, b in zip(_three_steps(g, "fp32", False), _three_steps(g, "fp32", True)):
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_two_runs_bit_identical(golden, prec):
    """Two runs of three captured steps leave bit-identical losses, parameters, moments and gradients."""
    g = golden("g24_train_newfluidnet_spectral")
    for a, b in zip(_three_steps(g, prec, True), _three_steps(g, prec, True)):
        assert torch.equal(a, b), float((a - b).abs().max())


def test_launch_budget(golden):
    """At most 3 launches per spectral layer forward before the GroupNorm launches, 3 backward (2 where the input needs no
    gradient: conv.0), and a captured step allocates nothing: the plan owns every buffer."""
    from pbml_mantle_convection_amd import _lib as L
    g = golden("g24_train_newfluidnet_spectral")
    m, tr = _trainer(g)
    gVTp, uvp = _batch(0)
    tr._fwd_bwd(gVTp, uvp, None, None, None, train=True)
    calls, real = [], L.call

    def spy(name, *a):
        if name.startswith("mc_spectral") and name != "mc_spectral_slots":
            calls.append(name)
        return real(name, *a)
    L.call = spy
    try:
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        eng = m.engine()
        params = tr.flat.views(tr.flat.param)
        eng.forward(gVTp, params, None, out=tr._ybuf)
        n_fwd = len(calls)
        eng.backward(torch.ones_like(tr._ybuf), params, tr.flat.views(tr.flat.grad))
        after = torch.cuda.memory_stats()["allocation.all.allocated"]
    finally:
        L.call = real
    layers = len(eng.spectral)
    assert layers == 4 and n_fwd == 3 * layers and len(calls) - n_fwd == 3 * layers - 1
    assert after - before <= 1, "forward / backward allocated device memory"      # (the ones_like above)


def test_cli_spectral(tmp_path):
    """The deployed configuration with -spectral 1 on synthetic data in a child process: exits 0 and writes a checkpoint whose
    complex weights load with strict=True."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet
    cmd = [sys.executable, "-m", "pbml_mantle_convection_amd.train", "-net", "newfluidnet", "-l", "5", "-f", "16", "-b", "16",
           "-p", "zeros", "-s", "0", "-ab", "10", "-r", "6", "-k", "5", "-l_sc", "1", "-spectral", "1", "--synthetic", "32", "128",
           "506", "--epochs", "1", "-gpu", "0", "--nn_root", str(tmp_path) + "/"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ck = glob.glob(str(tmp_path / "*" / "0_fluidnet_uvp.pt"))
    assert len(ck) == 1, os.listdir(tmp_path)
    sd = torch.load(ck[0], map_location="cpu", weights_only=True)
    m = NewFluidNet(5, 7, 16, 1, None, "gelu", "zeros", "curl", use_symm=False, a_bound=10, repeats=6, f=5, p_pred=False,
                    spectral_conv=True)
    m.load_state_dict(sd, strict=True)
    assert sd["conv.0.layers.0.weights1"].dtype == torch.complex64
    assert all(bool(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all()) for v in sd.values())

"""Channel widths that are not multiples of 8 on the HIP path: mc_concat_cb8 with unaligned operands and mc_cat_grad_gather
against torch, the c_h = 6 Unet (learned and replicate padding) and the c_h = 12 NewFluidNet against the reference
(golden g23), the 16-bit modes against fp32, the reference's roll-4 get_loss through Trainer (eager and captured), graph /
eager bit identity and the CLI end to end."""
import ctypes as C
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
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "mixed": torch.float16}


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype).to(DEV)


def assert_close(a, b, atol, rtol=1e-4, what=""):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b)
    tol = atol + rtol * np.abs(b)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e} (tol {atol}+{rtol}*|ref|), MAE {err.mean():.3e}"


def to_cb8(t, pad_value=0.0):
    """NCHW -> CB8 [N][C8][H][W][8] on the device, the lanes past C filled with pad_value."""
    n, c, h, w = t.shape
    c8 = (c + 7) // 8
    p = torch.full((n, c8 * 8, h, w), pad_value, dtype=t.dtype)
    p[:, :c] = t
    return p.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(DEV)


def bits(t):
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _concat(bufs, chans, N, H, W, prec, out):
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd.engine import DTYPES as MC
    srcs = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
    cs = (C.c_int32 * len(bufs))(*chans)
    L.call("mc_concat_cb8", srcs, cs, len(bufs), N, H, W, MC[prec][0], L.ptr(out), L.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "mixed"])
@pytest.mark.parametrize("chans", [[6, 6], [6, 12], [12, 24], [3, 5, 7], [12] * 5 + [7], [16, 16], [16, 8, 5]])
def test_concat_any_widths_vs_torch_cat(prec, chans):
    """Exact (bit for bit) against torch.cat; sources whose padding lanes hold NaN never leak them into a channel, and the
    output's padding lanes are zeros.  All-aligned operand lists ([16, 16], [16, 8, 5]) take the block-copy kernel of
    before: bit-identical to the whole-block copy of the operands (the last operand's padding lanes included)."""
    from pbml_mantle_convection_amd import _lib as L
    L.load()
    dt = DTYPES[prec]
    N, H, W = 2, 9, 37
    g = torch.Generator().manual_seed(sum(chans) * 31 + len(chans))
    xs = [torch.randn((N, c, H, W), generator=g).to(dt) for c in chans]
    aligned = all(c % 8 == 0 for c in chans[:-1])
    bufs = [to_cb8(x, 0.0 if aligned else float("nan")) for x in xs]
    C8 = (sum(chans) + 7) // 8
    out = torch.full((N, C8, H, W, 8), float("nan"), dtype=dt, device=DEV)
    _concat(bufs, chans, N, H, W, prec, out)
    ref = to_cb8(torch.cat(xs, 1), 0.0)
    assert torch.equal(bits(out), bits(ref))
    if aligned:
        whole = torch.cat([b.cpu() for b in bufs], 1)
        assert torch.equal(bits(out), bits(whole))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "mixed"])
@pytest.mark.parametrize("kind,pad,mode", [("plain", 0, "zeros"), ("padfold", 2, "zeros"), ("padfold", 2, "reflect"),
                                           ("padfold", 1, "replicate")])
def test_cat_grad_gather_vs_slice(prec, kind, pad, mode):
    """Every operand range of a [6, 12, 7] concat and of the trunk's [12, 12, 7]: channels [c_off, c_off + c) of the
    concatenated gradient (PLAIN: the tensor itself; PADFOLD: the interior of a padded domain), exact, padding lanes zero."""
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd.engine import DTYPES as MC
    L.load()
    gdt = torch.float32 if prec == "fp32" else torch.bfloat16                # gradient tensors: bf16 in the mixed mode
    mcg = L.MC_F32 if prec == "fp32" else L.MC_BF16
    assert MC[prec][0] in (mcg, L.MC_MIX16)
    N, H, W = 2, 11, 29
    for chans in ([6, 12, 7], [12, 12, 7]):
        ct = sum(chans)
        g = torch.Generator().manual_seed(ct * 7 + pad)
        full = torch.randn((N, ct, H + 2 * pad, W + 2 * pad), generator=g).to(gdt)
        buf = to_cb8(full, float("nan"))
        gs = L.GradSrc(L.ptr(buf), L.GSRC_PLAIN if kind == "plain" else L.GSRC_PADFOLD, pad, L.PAD_MODES[mode], 1, H, W)
        off = 0
        for c in chans:
            out = torch.full((N, (c + 7) // 8, H, W, 8), float("nan"), dtype=gdt, device=DEV)
            L.call("mc_cat_grad_gather", C.byref(gs), ct, off, c, N, H, W, mcg, L.ptr(out), L.stream())
            torch.cuda.synchronize()
            ref = to_cb8(full[:, off:off + c, pad:pad + H, pad:pad + W], 0.0)
            assert torch.equal(bits(out), bits(ref)), (chans, off, c)
            off += c


# ------------------------------------------------------------------ networks against the reference (golden g23)
def _grad_ref_cmp(got, ref):
    """Gradients of more than 512 entries are stored as fields.strided_sample(g, 257)."""
    got = got.detach().float().cpu().numpy()
    return (fields.strided_sample(got, 257) if ref.size != got.size else got.reshape(ref.shape)), ref


def _unet(g, prec="fp32"):
    from pbml_mantle_convection_amd.pytorch_networks_convae import Unet
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm = [int(v) for v in g["cfg"][:8]]
    m = Unet(levels, c_i, c_h, c_o, torch.device(DEV), "gelu", str(g["r_p"]) if "r_p" in g.files else "learned", "curl",
             use_symm=bool(symm), repeats=repeats, f=f, p_pred=bool(p_pred))
    m.load_state_dict({n[3:]: torch.from_numpy(g[n]).float() for n in g.files if n.startswith("sd/")}, strict=True)
    m = m.to(DEV)
    return m.set_precision(prec) if prec != "fp32" else m


def _unet_run(g, seed, prec="fp32"):
    m = _unet(g, prec)
    outs = m(dev(fields.unet_input(2, 40, 54, seed + 2, c_i=10)))
    loss, got = 0.0, {}
    for n, o in zip("uvpT", outs):
        if o is None:
            assert "out/" + n not in g.files
            continue
        got[n] = o
        loss = loss + (o * dev(g["ct/" + n])).sum()
    loss.backward()
    return m, got


@pytest.mark.parametrize("tag,seed", [("learned", 230), ("replicate", 235)])
def test_unet6_vs_golden(golden, tag, seed):
    """fp32 forward (u, v, T) and every parameter gradient of the c_h = 6 Unet (concats [6, 6] and [6, 12], GroupNorm with
    one group of 6 channels) against the reference, at the tolerances of test_unet_learned_padding_vs_golden.  replicate:
    the fixed-padding materialised concat and the PADFOLD gradient gather."""
    g = golden(f"g23_unet6_{tag}")
    m, got = _unet_run(g, seed)
    assert set(got) == {n[4:] for n in g.files if n.startswith("out/")}
    for n, o in got.items():
        ref = g["out/" + n]
        assert_close(o, ref, atol=3e-5 * max(1.0, float(np.abs(ref).max())), rtol=2e-4, what="out " + n)
    for n, p in m.named_parameters():
        a, ref = _grad_ref_cmp(p.grad, g["grad/" + n])
        if float(np.abs(ref).max()) < 1e-6:
            continue                                    # null directions (the last layer's shared bias under the zero-mean)
        assert_close(a, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=3e-3, what="grad " + n)


def test_newfluidnet12_vs_golden(golden):
    """NewFluidNet with c_h = 12 and learned padding: the trunk's [12, 12, 7] concat, its two gathered operand gradients."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet
    g = golden("g23_newfluidnet12_learned")
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm = [int(v) for v in g["cfg"]]
    m = NewFluidNet(levels, c_i, c_h, c_o, torch.device(DEV), "gelu", "learned", "curl", use_symm=bool(symm), repeats=repeats,
                    f=f, p_pred=bool(p_pred))
    m.load_state_dict({n[3:]: torch.from_numpy(g[n]).float() for n in g.files if n.startswith("sd/")}, strict=True)
    m = m.to(DEV)
    outs = m(dev(fields.unet_input(1, 128, 506, 239, c_i=c_i)))
    loss, k = 0.0, 0
    for n, o in zip("uvp", outs):
        if o is None:
            continue
        ref = g["out/" + n]
        assert_close(fields.strided_sample(o.detach().cpu().numpy(), 5003), ref, atol=3e-5 * max(1.0, float(np.abs(ref).max())),
                     rtol=2e-4, what="out " + n)
        loss = loss + (o * dev(fields.smooth_field(1, 128, 506, 240 + k).astype(np.float32)).view(o.shape)).sum()
        k += 1
    assert k == 2
    loss.backward()
    for n, p in m.named_parameters():
        a, ref = _grad_ref_cmp(p.grad, g["grad/" + n])
        if float(np.abs(ref).max()) < 1e-6:
            continue
        assert_close(a, ref, atol=5e-4 * max(1.0, float(np.abs(ref).max())), rtol=3e-3, what="grad " + n)


@pytest.mark.parametrize("prec", ["bf16", "mixed"])
def test_unet6_16bit_modes_near_golden(golden, prec):
    """The bounds of test_unet_learned_padding_bf16_vs_golden: output MAE <= 0.12 mean |ref|, gradient rel-L2 < 0.3."""
    g = golden("g23_unet6_learned")
    m, got = _unet_run(g, 230, prec)
    for n, o in got.items():
        ref = g["out/" + n]
        assert float(np.abs(o.detach().double().cpu().numpy() - ref).mean()) <= 0.12 * float(np.abs(ref).mean()), n
    num = den = 0.0
    for n, p in m.named_parameters():
        a, ref = _grad_ref_cmp(p.grad, g["grad/" + n])
        num += float(np.sum((a.astype(np.float64) - ref) ** 2))
        den += float(np.sum(ref.astype(np.float64) ** 2))
    assert (num / den) ** 0.5 < 0.3, (num / den) ** 0.5


# ------------------------------------------------------------------ training: roll-4 get_loss, graph capture, CLI
def _trainer(m, R=1, use_graph=False, lr=1e-3, prec="fp32"):
    from pbml_mantle_convection_amd.multigpu import Trainer
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1000], gamma=0.5)
    return Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=False, network="unet", loss_type="curl",
                   loss_scale=True, loss_derivative=True, roll_forward=R, precision=prec, use_graph=use_graph)


def _batch(B=1):
    H, W = 128, 506
    gVTp = dev(fields.unet_input(B, H, W, 2330, c_i=10))
    uvp = dev(np.stack([fields.smooth_field(B, H, W, 2331), fields.smooth_field(B, H, W, 2332),
                        fields.temperature_field(B, H, W, 2333)], 1))
    return gVTp, uvp


@pytest.mark.parametrize("path", ["get_loss", "graph"])
def test_roll_forward_4_golden(golden, path):
    """The run list's -roll 4 (4 x 4 chained evaluations) on the learned c_h = 6 Unet, loss_scale = loss_derivative = 1:
    the reference's six losses and every parameter gradient, through the autograd-visible get_loss and inside a captured
    step (replayed once more with lr 0)."""
    g = golden("g23_get_loss_unet6_roll4")
    R = int(g["cfg"][10])
    m = _unet(golden("g23_unet6_learned"))
    gVTp, uvp = _batch()
    paras = dev(g["paras"]).view(1, 3, 1, 1)
    g_in = gVTp.clone()
    if path == "get_loss":
        tr = _trainer(m, R)
        loss6 = tr.get_loss(gVTp, uvp, None, paras, gVTp[:, 1:2])
        loss6[0].backward()
        vals = torch.stack([v.detach().reshape(()) for v in loss6])
        grads = {n: p.grad for n, p in m.named_parameters()}
    else:
        tr = _trainer(m, R, use_graph=True, lr=0.0)
        for _ in range(2):
            out8 = tr.train_step(gVTp, uvp, None, paras, None)
        torch.cuda.synchronize()
        vals = out8[:6]
        grads = tr.flat.views(tr.flat.grad)
    assert torch.equal(gVTp, g_in), "the batch itself must not be written"
    assert_close(vals, g["losses"], atol=1e-6, rtol=1e-4, what="losses")
    for n, gr in grads.items():
        a, ref = _grad_ref_cmp(gr, g["grad/" + n])
        assert_close(a, ref, atol=3e-4 * max(1.0, float(np.abs(ref).max())), rtol=2e-3, what="grad " + n)


@pytest.mark.parametrize("tag", ["learned", "replicate"])
def test_captured_steps_bit_identical_to_eager(golden, tag):
    """Two HIP-graph-captured training steps of the c_h = 6 Unet leave the same parameters, Adam moments and losses as two
    eager ones."""
    gVTp, uvp = _batch(2)
    res = []
    for use_graph in (False, True):
        tr = _trainer(_unet(golden(f"g23_unet6_{tag}")), use_graph=use_graph)
        outs = [tr.train_step(gVTp, uvp).clone() for _ in range(2)]
        torch.cuda.synchronize()
        res.append((*outs, tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("net,extra", [
    ("unet", ["-l", "3", "-f", "6", "-r", "2", "-k", "5", "-p", "learned", "-roll", "1", "-l_sc", "1", "-l_de", "1"]),
    ("fluidnet", ["-l", "2", "-f", "12", "-r", "1", "-k", "5", "-p", "learned"]),
])
def test_cli_end_to_end(tmp_path, net, extra):
    """`-net unet -f 6` and `-net fluidnet -f 12` on synthetic data in a child process on one device: exits 0 and writes the
    reference-named checkpoint, which loads with strict=True into the reference-shaped module."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet, Unet
    cmd = [sys.executable, "-m", "pbml_mantle_convection_amd.train", "-net", net, "-b", "2", "-s", "0", "-ab", "10",
           "--synthetic", "4", "128", "506", "--epochs", "1", "-gpu", "0", "--nn_root", str(tmp_path) + "/"] + extra
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ck = glob.glob(str(tmp_path / "*" / "0_fluidnet_uvp.pt"))                 # (the reference names every checkpoint so)
    assert len(ck) == 1, os.listdir(tmp_path)
    sd = torch.load(ck[0], map_location="cpu", weights_only=True)
    if net == "unet":
        m = Unet(3, 10, 6, 2, None, "gelu", "learned", "curl", use_symm=False, a_bound=10, repeats=2, f=5, p_pred=False)
    else:
        m = FluidNet(2, 7, 12, 1, None, "gelu", "learned", "curl", use_symm=False, a_bound=10, repeats=1, f=5, p_pred=False)
    m.load_state_dict(sd, strict=True)
    assert all(bool(torch.isfinite(v).all()) for v in sd.values())

"""Dropout at the layer, network and trainer level.

The f64 oracle is oracle/ref_cpu.py with its `fluid_layer` wrapped (monkeypatch): the wrapper multiplies the layer's result by
the restated mask (tests/dropout_ref.py) times the scale, for that prefix's layer id; newfluidnet_features resolves the name
at call time and torch autograd gives the gradients.  fp32 gates are the project's: output within 2e-5 of
max|ref|, gradients at rtol 2e-3."""
import numpy as np
import pytest
import torch

import dropout_ref as R
import fields
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 0.1
SEED = (0x7F4A7C15 << 32) | 0x9E3779B9
KEY = (SEED & 0xFFFFFFFF, SEED >> 32)


def npy(t):
    return t.detach().cpu().double().numpy()


def grad_gate(got, ref, what):
    """The project's fp32 gate for a gradient tensor: rtol 2e-3 on a floor of 3e-4 of the tensor's scale."""
    got, ref = npy(got), npy(ref)
    assert got.shape == ref.shape, what
    err = np.abs(got - ref)
    tol = 3e-4 * max(1.0, float(np.abs(ref).max())) + 2e-3 * np.abs(ref)
    assert (err <= tol).all(), f"{what}: max err {err.max():.3e} (ref max {np.abs(ref).max():.3e})"


def mask_scale(step, layer, shape):
    n, c, h, w = shape
    keep = R.keep_nchw(KEY, step, layer, n, c, h, w, R.keep16(P))
    return torch.from_numpy(keep.astype(np.float64) * float(R.scale(P)))


def draw(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


# ---- stand-alone FluidLayer ---------------------------------------------------------------------------------------------------
def _layer(r_p, drop):
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidLayer
    torch.manual_seed(11)
    m = FluidLayer(4, 8, "gelu", r_p, use_symm=True, f=5, drop_rate=drop)
    with torch.no_grad():
        m.layers[1].weight.add_(0.2 * torch.randn(8))
        m.layers[1].bias.add_(0.2 * torch.randn(8))
    return m


def _layer_ref(sd, x, r_p, ms):
    if r_p == "learned":
        y = O.boundary_learned_conv(sd, "layers.0.", x, 5, True)
        y = torch.nn.functional.group_norm(y, O.gn_groups(8), sd["layers.1.weight"], sd["layers.1.bias"], 1e-5)
        a = O.activation("gelu", y)
    else:
        a = O.fluid_layer(sd, "", x, "gelu", r_p, True)
    return a * ms


@pytest.mark.parametrize("r_p,shape", [("zeros", (2, 4, 20, 24)),         # one-launch GroupNorm kernels
                                       ("replicate", (2, 4, 72, 80)),     # three-phase path
                                       ("learned", (2, 4, 24, 28))],      # behind a learned-padding conv, with dx
                         ids=["small", "three-phase", "learned"])
def test_fluid_layer_against_masked_oracle(r_p, shape):
    m = _layer(r_p, P).to(DEV).train()
    m.set_dropout_seed(SEED)
    x = draw(shape, 21)
    ct = draw((shape[0], 8, shape[2], shape[3]), 22)
    xd = x.to(DEV).requires_grad_(r_p == "learned")
    y = m(xd)
    (y * ct.to(DEV)).sum().backward()
    assert m.engine().dropout_step() == 1
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    ref = _layer_ref(sd, x64, r_p, mask_scale(1, 0, tuple(y.shape)))
    (ref * ct.double()).sum().backward()
    err = float((y.detach().cpu().double() - ref.detach()).abs().max())
    scale = float(ref.detach().abs().max())
    print(f"{r_p} {shape}: output err {err:.3e} = {err / scale:.2e} of max|ref|")
    assert err <= 2e-5 * scale
    dropped = (ref.detach() == 0)
    assert 0.05 < float(dropped.double().mean()) < 0.15
    assert bool((y.detach().cpu()[dropped] == 0).all())
    for n, p in m.named_parameters():
        grad_gate(p.grad, sd[n].grad, "grad " + n)
    if r_p == "learned":
        grad_gate(xd.grad, x64.grad, "dx")


def test_fluid_layer_modes_and_seeding():
    m = _layer("zeros", P).to(DEV)
    twin = _layer("zeros", 0.0).to(DEV)
    twin.load_state_dict(m.state_dict())
    x = draw((2, 4, 20, 24), 23).to(DEV)
    m.eval()
    assert torch.equal(m(x), twin(x)), "eval mode differs from the drop-free layer"
    m.train()
    with torch.no_grad():
        assert torch.equal(m(x), twin(x)), "a forward under no_grad draws no mask"
    m.set_dropout_seed(SEED)
    a, b = m(x).detach().clone(), m(x).detach().clone()
    assert not torch.equal(a, b), "two training forwards drew the same mask"
    assert m.engine().dropout_step() == 2
    m.set_dropout_seed(SEED)
    assert torch.equal(m(x).detach(), a), "re-seeding does not reproduce the first forward"
    m.set_dropout_seed(SEED + 1)
    assert not torch.equal(m(x).detach(), a)
    m.set_precision("bf16")                         # an engine created later takes the module's seed
    m.set_dropout_seed(SEED)
    c = m(x).detach()
    assert bool(((c == 0) == (a == 0)).all()), "the mask depends on the precision"


# ---- NewFluidNet ------------------------------------------------------------------------------------------------------------
CFG = dict(levels=2, c_i=7, c_h=8, c_o=3, repeats=2)
NET_SHAPE = (2, 7, 72, 80)            # level 0 takes the three-phase path, level 1 (36 x 40) the one-launch kernels


def _net(drop, prec="fp32"):
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet
    torch.manual_seed(12)
    m = NewFluidNet(2, 7, 8, 3, None, "gelu", "zeros", "mae", use_symm=True, repeats=2, f=5, p_pred=True, drop_rate=drop)
    return m.to(DEV).set_precision(prec)


def _patched_oracle(monkeypatch, step):
    ids = {row[0]: i for i, row in enumerate(O.newfluidnet_layer_table(CFG["levels"], 7, 8, 3, CFG["repeats"]))}
    orig = O.fluid_layer

    def wrapped(sd, prefix, x, act, r_p, use_symm):
        a = orig(sd, prefix, x, act, r_p, use_symm)
        return a * mask_scale(step, ids[prefix], tuple(a.shape))
    monkeypatch.setattr(O, "fluid_layer", wrapped)


@pytest.fixture(scope="module")
def net_input():
    return torch.from_numpy(fields.unet_input(NET_SHAPE[0], NET_SHAPE[2], NET_SHAPE[3], 501, c_i=7)).float()


def _oracle_run(monkeypatch, m, x, cts):
    _patched_oracle(monkeypatch, 1)
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in m.state_dict().items()}
    ref = O.newfluidnet_forward(sd, x.double(), levels=2, repeats=2, act="gelu", r_p="zeros", loss_type="mae", use_symm=True,
                                p_pred=True)
    sum((r * c.double()).sum() for r, c in zip(ref, cts)).backward()
    return sd, ref


def test_newfluidnet_fp32_against_masked_oracle(monkeypatch, net_input):
    m = _net(P).train()
    m.set_dropout_seed(SEED)
    outs = m(net_input.to(DEV))
    cts = [draw(tuple(o.shape), 31 + i) for i, o in enumerate(outs)]
    sum((o * c.to(DEV)).sum() for o, c in zip(outs, cts)).backward()
    sd, ref = _oracle_run(monkeypatch, m, net_input, cts)
    for n, o, r in zip("uvp", outs, ref):
        err = float((o.detach().cpu().double() - r.detach()).abs().max())
        print(f"newfluidnet fp32 out {n}: err {err:.3e} = {err / float(r.abs().max()):.2e} of max|ref|")
        assert err <= 2e-5 * float(r.abs().max()), n
    for n, p in m.named_parameters():
        if float(sd[n].grad.abs().max()) < 1e-6:
            continue                                    # null direction (the last conv's bias under the zero-mean)
        grad_gate(p.grad, sd[n].grad, "grad " + n)


# forward relative L2 against the masked f64 oracle: 1.5 x what MI355X measured
L2_MEASURED = {"bf16": 1.1285e-2, "mixed": 1.4441e-3}


@pytest.mark.parametrize("prec", ["bf16", "mixed"])
def test_newfluidnet_16bit_against_masked_oracle(monkeypatch, net_input, prec):
    m = _net(P, prec).train()
    m.set_dropout_seed(SEED)
    outs = m(net_input.to(DEV))
    _patched_oracle(monkeypatch, 1)
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    ref = O.newfluidnet_forward(sd, net_input.double(), levels=2, repeats=2, act="gelu", r_p="zeros", loss_type="mae",
                                use_symm=True, p_pred=True)
    o = np.concatenate([npy(t).reshape(-1) for t in outs])
    r = np.concatenate([npy(t).reshape(-1) for t in ref])
    rel = float(np.linalg.norm(o - r) / np.linalg.norm(r))
    print(f"newfluidnet {prec}: forward rel-L2 {rel:.4e}")
    assert np.isfinite(rel)
    assert rel <= 1.5 * L2_MEASURED[prec], rel


@pytest.mark.parametrize("fuse", ["0", "3"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "mixed"])
def test_dropout_nodes_are_materialised_and_keep_their_own_backward(monkeypatch, prec, fuse):
    """No dropout node is planned `fused` or receives the dz epilogue of its consumer's input-gradient launch -- also where
    the engine is told to fuse everything it can (MANTLE_FUSE=3), which does fuse the drop-free twin."""
    from pbml_mantle_convection_amd.engine import Engine
    monkeypatch.setenv("MANTLE_FUSE", fuse)
    found = {}
    for drop in (P, 0.0):
        g = _net(drop)._graph
        eng = Engine(g, prec)
        eng.configure(*NET_SHAPE[:1], *NET_SHAPE[2:], torch.device(DEV))
        trunk = [e for e in eng.plan if e.node.kind == "conv" and e.node.name.startswith(("conv.0.", "convs."))]
        assert len(trunk) == 5
        found[drop] = [(eng.T[e.node.out].fused, e.route.dz_blocks > 0, any(o.route.epi >= 0 and eng.plan[o.route.epi] is e for o in eng.convs)) for e in trunk]
        if drop:
            assert all(e.node.drop == P for e in trunk)
            assert eng.drop_state is not None and eng.T[trunk[0].node.out].buf is not None
        else:
            assert eng.drop_state is None
    assert not any(any(t) for t in found[P]), found[P]
    if fuse == "3":
        assert any(any(t) for t in found[0.0]), "the twin fuses nothing: the check above shows nothing"


# ---- Trainer ----------------------------------------------------------------------------------------------------------------
def _trainer(drop, use_graph, seed=1234, prec="bf16", state=None):
    from pbml_mantle_convection_amd.multigpu import Trainer
    m = _net(drop)
    if state is not None:
        m.load_state_dict(state)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.5)
    tr = Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="newfluidnet", loss_scale=True,
                 loss_type="mae", precision=prec, use_graph=use_graph, drop_seed=seed)
    return m, tr


@pytest.fixture(scope="module")
def batch(net_input):
    B, _, H, W = NET_SHAPE
    uvp = np.stack([fields.smooth_field(B, H, W, 511), fields.smooth_field(B, H, W, 512), fields.smooth_field(B, H, W, 513, amp=0.5)], 1)
    return net_input.to(DEV), torch.from_numpy(uvp).float().to(DEV)


def _three_steps(batch, use_graph, seed=1234):
    m, tr = _trainer(P, use_graph, seed)
    outs = [tr.train_step(*batch).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert m.engine().dropout_step() == 3, "the device step counter must read 3 (the capture's warm-up consumes none)"
    return (*outs, tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.flat.grad.clone()), (m, tr)


def test_trainer_captured_equals_eager_and_runs_repeat(batch):
    eager, _ = _three_steps(batch, False)
    graph, (m, tr) = _three_steps(batch, True)
    again, _ = _three_steps(batch, True)
    for name, a, b, c in zip(["out0", "out1", "out2", "param", "exp_avg", "exp_avg_sq", "grad"], eager, graph, again):
        assert torch.equal(a, b), f"{name}: captured differs from eager by {float((a - b).abs().max()):.3e}"
        assert torch.equal(b, c), f"{name}: two captured runs differ"
    assert not torch.equal(eager[0], eager[1]) or not torch.equal(eager[1], eager[2])
    other, _ = _three_steps(batch, True, seed=1235)
    assert not torch.equal(other[3], graph[3]), "another seed left the same parameters"
    # evaluation draws no mask: bit for bit the drop-free model holding the same weights
    m0, tr0 = _trainer(0.0, False, state=m.state_dict())
    assert torch.equal(tr.eval_step(*batch), tr0.eval_step(*batch))
    assert m.engine().dropout_step() == 3


def test_trainer_seed_carries_rank_and_epoch(batch):
    from pbml_mantle_convection_amd.multigpu import dropout_seed
    m, tr = _trainer(P, False, seed=77)
    assert tr.drop_seed == dropout_seed(77, 0, 0) and m._drop_seed == tr.drop_seed


# ---- FluidNet ---------------------------------------------------------------------------------------------------------------
def test_fluidnet_learned_curl_trains_and_evaluates():
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet

    def make(drop):
        torch.manual_seed(13)
        return FluidNet(2, 7, 8, 1, None, "gelu", "learned", "curl", use_symm=True, a_bound=10.0, repeats=2, f=5, p_pred=False,
                        drop_rate=drop).to(DEV)
    m, twin = make(P), make(0.0)
    B, H, W = 2, 40, 48
    x = torch.from_numpy(fields.unet_input(B, H, W, 521, c_i=7)).float().to(DEV)
    m.eval()
    with torch.no_grad():
        for a, b in zip(m(x)[:2], twin(x)[:2]):
            assert torch.equal(a, b)
    uvp = torch.from_numpy(np.stack([fields.smooth_field(B, H, W, 522), fields.smooth_field(B, H, W, 523)], 1)).float().to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.5)
    tr = Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=False, network="fluidnet", loss_type="curl",
                 precision="fp32", drop_seed=5)
    before = tr.flat.param.clone()
    out = tr.train_step(x, uvp)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tr.flat.param).all())
    assert not torch.equal(before, tr.flat.param)
    assert m.engine().dropout_step() == 1
    ev = tr.eval_step(x, uvp)
    opt0 = torch.optim.Adam(twin.parameters(), lr=1e-3)
    twin.load_state_dict(m.state_dict())
    tr0 = Trainer(twin, None, None, None, None, None, opt0, torch.optim.lr_scheduler.MultiStepLR(opt0, milestones=[100]), 0, 1,
                  "/tmp/", p_pred=False, network="fluidnet", loss_type="curl", precision="fp32")
    assert torch.equal(ev, tr0.eval_step(x, uvp))

"""Host-side checks of the spectral layers (no GPU): the f64 restatement in tests/spectral_ref.py against the reference's own
layer (g24), the module tree and the flat parameter store with complex parameters, the graph wiring, the shape limits, the
twiddle tables, and that the comparison the kernel tests use can see a wrong kernel."""
import numpy as np
import pytest
import torch

import spectral_ref as R
from pbml_mantle_convection_amd import engine as E
from pbml_mantle_convection_amd.hipnet import FlatParams
from pbml_mantle_convection_amd.pytorch_networks_convae import (FluidNet, NewFluidNet, SpectralConv2d, SpectralFluidLayer, Unet,
                                                                count_parameters)

c128 = torch.complex128


def _layer_case(g, tag):
    t = lambda k, dt=torch.float64: torch.from_numpy(g[f"{tag}/{k}"]).to(dt)  # noqa: E731
    return (t("x"), t("sd/layers.0.weights1", c128), t("sd/layers.0.weights2", c128), t("sd/layers.1.weight"), t("sd/layers.1.bias"),
            str(g[f"{tag}/act"]))


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_reproduces_the_reference_layer(golden, tag):
    """tests/spectral_ref.py against the reference's SpectralFluidLayer in f64: output, dx and every parameter gradient to 1e-9
    (relative to the largest reference entry of each array)."""
    g = golden("g24_spectral_layer")
    x, w1, w2, gw, gb, act = _layer_case(g, tag)
    leaves = [v.clone().requires_grad_(True) for v in (x, w1, w2, gw, gb)]
    y = R.layer_torch(*leaves, act)
    (y * torch.from_numpy(g[f"{tag}/ct"]).double()).sum().backward()
    pairs = [("y", y.detach(), g[f"{tag}/y"]), ("dx", leaves[0].grad, g[f"{tag}/dx"])]
    pairs += [("grad " + n, leaf.grad, g[f"{tag}/grad/{n}"]) for n, leaf in zip(
        ("layers.0.weights1", "layers.0.weights2", "layers.1.weight", "layers.1.bias"), leaves[1:])]
    for what, got, ref in pairs:
        err = np.abs(got.numpy() - ref).max()
        assert err <= 1e-9 * max(1.0, np.abs(ref).max()), f"{tag} {what}: {err:.3e}"


@pytest.mark.parametrize("tag", ["a", "b"])
def test_explicit_backward_formulas(golden, tag):
    """The closed forms of the two linear maps' backward (what the kernels compute) against autograd through the dense
    restatement, on the convolution alone."""
    g = golden("g24_spectral_layer")
    x, w1, w2, _, _, _ = _layer_case(g, tag)
    H, W = x.shape[-2:]
    y = R.conv_fwd(x.numpy(), w1.numpy(), w2.numpy())
    dy = R.draw(y.shape, 7)
    xt, w1t, w2t = (v.clone().requires_grad_(True) for v in (x, w1, w2))
    E1, E2 = (torch.from_numpy(e) for e in R.phases_exact(H, W))
    co = torch.einsum("nikq,iokq->nokq", torch.einsum("nchw,kh,qw->nckq", xt.to(c128), E1, E2),
                      torch.cat([w1t, w2t], 2)) * torch.from_numpy(R.gamma(H, W))
    yt = torch.einsum("nckq,kh,qw->nchw", co, E1.conj(), E2.conj()).real
    assert np.abs(yt.detach().numpy() - y).max() <= 1e-13 * max(1.0, np.abs(y).max())
    # the reference's rfft2 / irfft2 form gives the same values
    ft = torch.fft.rfft2(x)
    out = torch.zeros((x.shape[0], w1.shape[1], H, W // 2 + 1), dtype=c128)
    out[:, :, :4, :4] = torch.einsum("bixy,ioxy->boxy", ft[:, :, :4, :4], w1)
    out[:, :, -4:, :4] = torch.einsum("bixy,ioxy->boxy", ft[:, :, -4:, :4], w2)
    assert np.abs(torch.fft.irfft2(out, s=(H, W)).numpy() - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    (yt * torch.from_numpy(dy)).sum().backward()
    dx, d1, d2 = R.conv_bwd(x.numpy(), w1.numpy(), w2.numpy(), dy)
    for what, got, ref in (("dx", dx, xt.grad.numpy()), ("dw1", d1, w1t.grad.numpy()), ("dw2", d2, w2t.grad.numpy())):
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what


# ---------------------------------------------------------------------------------------------- (b)
def _nets():
    return {"g24_newfluidnet_spectral": lambda: NewFluidNet(5, 7, 8, 3, None, "gelu", "zeros", "mae", use_symm=True, repeats=1, f=5,
                                                            p_pred=True, spectral_conv=True),
            "g24_fluidnet_spectral": lambda: FluidNet(2, 7, 8, 1, None, "gelu", "learned", "curl", use_symm=True, a_bound=10,
                                                      repeats=1, f=5, p_pred=False, spectral_conv=True)}


@pytest.mark.parametrize("name", list(_nets()))
def test_module_tree_matches_the_reference(golden, name):
    """state_dict keys (in order), shapes, which entries are complex, and count_parameters equal what the reference built."""
    g = golden(name)
    m = _nets()[name]()
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert [v.is_complex() for v in sd.values()] == ["complex" in str(d) for d in g["dtypes"]]
    assert all(v.dtype == torch.complex64 for v in sd.values() if v.is_complex())      # f32 masters
    assert count_parameters(m) == int(g["count"])
    if name == "g24_newfluidnet_spectral":
        assert count_parameters(m) == 16339
    assert isinstance(m.conv[0], SpectralFluidLayer) and isinstance(m.convs[0][0].layers[0], SpectralConv2d)
    w = m.conv[0].layers[0].weights1.detach()
    s = m.conv[0].layers[0].scale
    assert float(w.real.min()) >= 0 and float(w.imag.min()) >= 0 and float(w.real.max()) <= s and float(w.imag.max()) <= s


# ---------------------------------------------------------------------------------------------- (c)
def test_flat_params_with_complex_parameters():
    torch.manual_seed(0)
    m = NewFluidNet(2, 7, 8, 3, None, "gelu", "zeros", "mae", use_symm=True, repeats=1, f=5, p_pred=True, spectral_conv=True)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    fp = FlatParams(m, "cpu")
    off = 0
    for (n, p), o, shp, cplx in zip(m.named_parameters(), fp.offsets, fp.shapes, fp.complex):
        assert o == (off + 3) // 4 * 4 and o % 4 == 0
        size = p.numel() * (2 if p.is_complex() else 1)
        off = o + size
        assert cplx == p.is_complex() and int(np.prod(shp)) == size
        assert torch.equal(p.detach(), before[n]), n
        assert p.data_ptr() == fp.param.data_ptr() + 4 * o and p.grad.data_ptr() == fp.grad.data_ptr() + 4 * o
        assert p.dtype == before[n].dtype and p.grad.dtype == p.dtype and p.grad.shape == p.shape
    assert fp.numel == (off + 3) // 4 * 4 and fp.bound()
    views, gviews = fp.views(fp.param), fp.views(fp.grad)
    n = "conv.0.layers.0.weights1"
    p = dict(m.named_parameters())[n]
    assert tuple(views[n].shape) == tuple(p.shape) + (2,) and views[n].dtype == torch.float32
    assert torch.equal(torch.view_as_complex(views[n]), p.detach())
    # writing the flat buffer changes p; the engine's accumulation into the flat gradient is p.grad
    o = fp.offsets[fp.names.index(n)]
    fp.param[o] = 3.0
    fp.param[o + 1] = -4.0
    assert complex(p.detach().reshape(-1)[0]) == complex(3.0, -4.0)
    gviews[n][0, 0, 0, 0, 1] += 2.5
    assert complex(p.grad.reshape(-1)[0]) == complex(0.0, 2.5)
    # a net without complex parameters is laid out as before: consecutive 16-byte aligned slices of numel floats
    m2 = NewFluidNet(2, 7, 8, 3, None, "gelu", "zeros", "mae", use_symm=True, repeats=1, f=5, p_pred=True)
    fp2 = FlatParams(m2, "cpu")
    off = 0
    for p, o, shp in zip(m2.parameters(), fp2.offsets, fp2.shapes):
        assert o == (off + 3) // 4 * 4 and shp == tuple(p.shape)
        off = o + p.numel()


def test_adam_on_interleaved_floats_is_complex_adam():
    """What the flat Adam kernel does to a complex parameter's (re, im) floats is what torch.optim.Adam does to the complex
    tensor."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(5, 3, generator=g, dtype=torch.float64) + 1j * torch.randn(5, 3, generator=g, dtype=torch.float64)
    gr = [torch.randn(5, 3, 2, generator=g, dtype=torch.float64) for _ in range(3)]
    pc = torch.nn.Parameter(w.clone())
    pr = torch.nn.Parameter(torch.view_as_real(w).clone())
    oc, orr = torch.optim.Adam([pc], lr=1e-2), torch.optim.Adam([pr], lr=1e-2)
    for gi in gr:
        pc.grad, pr.grad = torch.view_as_complex(gi).clone(), gi.clone()
        oc.step()
        orr.step()
    assert torch.allclose(torch.view_as_real(pc.detach()), pr.detach(), rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("builder", [E.newfluidnet_graph, E.fluidnet_graph])
@pytest.mark.parametrize("r_p", ["zeros", "learned"])
def test_graph_wiring(builder, r_p):
    kw = dict(act="gelu", r_p=r_p, use_symm=True, repeats=2, f=5)
    gs, gc = builder(3, 7, 8, 1, spectral=True, **kw), builder(3, 7, 8, 1, **kw)
    assert gs.channels == gc.channels and len(gs.nodes) == len(gc.nodes)
    trunk = 0
    for a, b in zip(gs.nodes, gc.nodes):
        assert a.kind == b.kind
        if a.kind == "conv":
            assert (a.name, a.srcs, a.out, a.c_out, a.post, a.gn_name, a.pool, a.pooled) == \
                   (b.name, b.srcs, b.out, b.c_out, b.post, b.gn_name, b.pool, b.pooled)
            if a.spectral:
                trunk += 1
                assert (a.k, a.pad, a.sym_h, a.sym_v, a.sym_hv, a.learned) == (0, 0, 0, 0, 0, False)
                assert a.groups == int(a.c_out / 4) and a.name.endswith("layers.0.")
            else:
                assert (a.k, a.pad, a.sym_h, a.learned, a.groups) == (b.k, b.pad, b.sym_h, b.learned, b.groups)
        elif a.kind == "cat":
            assert (a.srcs, a.out) == (b.srcs, b.out)
        else:
            assert (a.src, a.out) == (b.src, b.out)
    assert trunk == 1 + 3 * 2
    names = [n for n, _, _ in E.iter_conv_descs(gs, 2, 64, 96, "fp32")]
    assert names and all(n.startswith(("conv.1.", "conv.2.", "conv.3.")) for n in names)      # the head convs only
    assert {n.split(".")[1] for n in names} == {"1", "2", "3"}
    size, grad, convs = E.shape_walk(gs, 2, 64, 96, "fp32")
    assert size == E.shape_walk(gc, 2, 64, 96, "fp32")[0]


def test_single_layer_graph_spectral():
    g = E.single_layer_graph(6, 12, 0, 0, "zeros", 0, E.L.POST_GN_ACT, "tanh", 3, gn=True, spectral=True, input_grad=True)
    (node,) = g.nodes
    assert node.spectral and g.input_grad and node.name == "layers.0." and node.gn_name == "layers.1."
    assert E.shape_walk(g, 2, 9, 11, "bf16")[1][0] is True


# ---------------------------------------------------------------------------------------------- (e)
def test_shape_limits():
    g = E.newfluidnet_graph(5, 7, 8, 3, act="gelu", r_p="zeros", use_symm=True, repeats=1, f=5, spectral=True)
    E.shape_walk(g, 1, 128, 506, "fp32")                       # 8 x 31 at the coarsest level: the minimum, allowed
    with pytest.raises(ValueError, match=r"convs\.4\.0\.layers\.0\..*7x31"):
        E.shape_walk(g, 1, 112, 506, "fp32")
    with pytest.raises(ValueError, match=r"convs\.4\.0\.layers\.0\..*8x7"):
        E.shape_walk(g, 1, 128, 112, "fp32")
    with pytest.raises(ValueError, match="c_o >= 4"):
        SpectralFluidLayer(4, 3, "gelu")
    with pytest.raises(NotImplementedError):
        Unet(3, 10, 8, 3, spectral_conv=True)
    with pytest.raises(NotImplementedError):                   # fixed padding keeps the trunk's c_h % 8 rule
        NewFluidNet(2, 7, 12, 3, None, "gelu", "zeros", "mae", spectral_conv=True)


# ---------------------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("H,W", [(8, 8), (9, 11), (8, 31), (37, 300), (128, 506), (506, 512)])
def test_twiddle_tables(H, W):
    row, col = E.spectral_tables(H, W)
    assert row.shape == (H, 5, 2) and col.shape == (W, 4, 2) and row.dtype == np.float32 and col.dtype == np.float32
    for tab, n in ((row, H), (col, W)):
        for j in range(n):
            for k in range(tab.shape[1]):
                a = 2.0 * np.pi * ((k * j) % n) / n
                assert tab[j, k, 0] == np.float32(np.cos(a)) and tab[j, k, 1] == np.float32(np.sin(a))
    r64, c64 = R.tables64(H, W)
    assert np.array_equal(row, r64.astype(np.float32)) and np.array_equal(col, c64.astype(np.float32))
    # the phases the kernels build from the tables are the exact ones to f32 rounding
    E1, E2 = R.phases_from_tables(row, col)
    X1, X2 = R.phases_exact(H, W)
    assert np.abs(E1 - X1).max() <= 2.0 ** -24 and np.abs(E2 - X2).max() <= 2.0 ** -24


# ---------------------------------------------------------------------------------------------- (g)
def _exceeds(got, ref, tol):
    return bool((np.abs(got - ref) > tol).any())


@pytest.mark.parametrize("H,W,c", R.CASES)
def test_kernel_comparison_sees_wrong_transforms(H, W, c):
    """On every case of the kernel tests' table, with their draws and their bound (the loosest store type, bf16, for the
    synthesis), these wrong kernels fail somewhere: e^{+i theta} in the analysis, the row-twiddle table shifted by one row,
    K1 taken as 0..7.  At H = 8 the list K1 = (0, 1, 2, 3, H-4 .. H-1) IS 0..7, so that variant is the same operator there
    (checked); it is seen at every other height."""
    E1, E2 = R.phases_exact(H, W)
    t = R.draw((R.CASE_N, c, H, W), 11, "bf16")
    ref = R.analysis(t, E1, E2)
    tol = R.bound(np.stack([ref.real, ref.imag], -1), R.analysis_abs(t, E1, E2))
    C = R.draw_complex((R.CASE_N, c, 8, 4), 12)
    sref = R.synthesis(C, E1, E2)
    stol = R.bound(sref, R.synthesis_abs(C, E1, E2), "bf16")

    def a_wrong(P1, P2):
        a = R.analysis(t, P1, P2)
        return _exceeds(np.stack([a.real, a.imag], -1), np.stack([ref.real, ref.imag], -1), tol)

    assert not a_wrong(E1, E2)
    assert a_wrong(*R.phases_exact(H, W, sign=+1.0)), "e^{+i theta}"
    S1, S2 = R.phases_exact(H, W, row_shift=1)
    assert a_wrong(S1, S2), "row table shifted (analysis)"
    assert _exceeds(R.synthesis(C, S1, S2), sref, stol), "row table shifted (synthesis)"
    K1, K2 = R.phases_exact(H, W, k1=list(range(8)))
    if H == 8:
        assert np.array_equal(K1, E1)
    else:
        assert a_wrong(K1, K2), "K1 = 0..7 (analysis)"
        assert _exceeds(R.synthesis(C, K1, K2), sref, stol), "K1 = 0..7 (synthesis)"


@pytest.mark.parametrize("H,W,c", R.CASES)
@pytest.mark.parametrize("ci,co", R.MIX_CASES)
def test_kernel_comparison_sees_wrong_mixing(H, W, c, ci, co):
    """... and in mode space: weights1 and weights2 swapped, gamma without the factor 2 (the grid size enters through
    gamma only)."""
    xhat = R.draw_complex((R.MIX_N, ci, 8, 4), 21)
    w1, w2 = R.draw_complex((ci, co, 4, 4), 22), R.draw_complex((ci, co, 4, 4), 23)
    gam = R.gamma(H, W)
    ref = R.mix_fwd(xhat, R.wt(w1, w2), gam)
    ref2 = np.stack([ref.real, ref.imag], -1)
    tol = R.bound(ref2, R.mix_fwd_abs(xhat, R.wt(w1, w2), gam))
    for what, got in (("swapped", R.mix_fwd(xhat, R.wt(w2, w1), gam)), ("gamma", R.mix_fwd(xhat, R.wt(w1, w2), R.gamma(H, W, False)))):
        assert _exceeds(np.stack([got.real, got.imag], -1), ref2, tol), what


# ---------------------------------------------------------------------------------------------- restart
def test_restart_keeps_complex_weights(tmp_path):
    """load_train_objs(restart=True) maps a checkpoint's entries to the f32 masters: real -> f32, complex -> complex64 (a
    checkpoint written in f64 / complex128, as the reference's are, included)."""
    from pbml_mantle_convection_amd import multigpu as G
    torch.manual_seed(1)
    src = NewFluidNet(2, 7, 8, 3, None, "gelu", "zeros", "mae", use_symm=False, repeats=1, f=5, p_pred=True, spectral_conv=True)
    d = str(tmp_path) + "/"
    with open(d + "fluidnet_uvpT.txt", "w") as f:
        f.write("Epoch, train loss, val loss, learning rate \n3, 0.1, 0.2, 0.0005\n")
    torch.save({k: v.to(torch.complex128) if v.is_complex() else v.double() for k, v in src.state_dict().items()},
               d + "3_fluidnet_uvp.pt")
    out = G.load_train_objs("cpu", 1, d, "", 2, 7, 8, 3, "gelu", "zeros", "mae", False, 1, 5, [20, 40], {}, {}, {}, {}, p_pred=True,
                            spectral_conv=True, restart=True, network="newfluidnet", synthetic=dict(n=2, H=16, W=24))
    m, epoch = out[2], out[6]
    assert epoch == 4
    for (n, a), (_, b) in zip(src.state_dict().items(), m.state_dict().items()):
        assert a.dtype == b.dtype and torch.equal(a, b), n
    assert m.conv[0].layers[0].weights1.dtype == torch.complex64


def test_synthetic_dataset_newfluidnet_items():
    """`-net newfluidnet --synthetic`: the FluidNet-family items (7 input channels, truth (u, v[, p]), a dummy weight, the
    scaler), as for 'fluidnet' -- the reference's `"fluidnet" in self.net` covers all three names."""
    from pbml_mantle_convection_amd.datasetio import SyntheticMantleDataset
    for p_pred, cy in ((True, 3), (False, 2)):
        ds = SyntheticMantleDataset(3, 24, 40, p_pred=p_pred, seed=5, network="newfluidnet", c_i=7)
        ref = SyntheticMantleDataset(3, 24, 40, p_pred=p_pred, seed=5, network="fluidnet", c_i=7)
        item = ds[1]
        assert len(item) == 4 and tuple(item[0].shape) == (7, 24, 40) and tuple(item[1].shape) == (cy, 24, 40)
        assert all(torch.equal(torch.as_tensor(a), torch.as_tensor(b)) for a, b in zip(item, ref[1]))

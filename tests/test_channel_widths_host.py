"""Channel widths that are not multiples of 8 (the run list's `-net unet -f 6`, FluidNet-family `-f 12`) on the host side:
the graphs, their shape walk and convolution descriptors, the plan's gradient buffers for unaligned concat operands, the
GroupNorm path choice at 6 channels per group, the module trees against the reference (golden g23) and the new C entry
point's argument validation.  No GPU."""
import ctypes as C

import pytest
import torch

MODES = ["learned", "zeros", "reflect", "replicate"]


def _graphs():
    from pbml_mantle_convection_amd import engine as E
    out = {f"unet6 {r_p}": (E.unet_graph(5, 10, 6, 2, act="gelu", r_p=r_p, use_symm=False, repeats=3, f=5), 16, 128, 506)
           for r_p in MODES}
    for c_h in (6, 12):
        out[f"newfluidnet{c_h} learned"] = (E.newfluidnet_graph(5, 7, c_h, 1, act="gelu", r_p="learned", use_symm=False,
                                                                repeats=4, f=5), 16, 128, 506)
        out[f"fluidnet{c_h} learned"] = (E.fluidnet_graph(5, 7, c_h, 1, act="gelu", r_p="learned", use_symm=False, repeats=4,
                                                          f=5), 16, 128, 506)
    return out


def test_unaligned_graphs_walk_and_every_launch_is_supported_and_in_bounds():
    """Every convolution launch of the c_h = 6 Unets and the c_h = 12 FluidNets, in every precision: a supported
    configuration, and the kernel's reach into its packed filter bank inside the bank (the guard of
    test_every_launch_reads_inside_its_filter_bank_and_workspaces)."""
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import engine as E
    lib = L.load()
    checked = 0
    for gname, (g, N, H, W) in _graphs().items():
        for prec in ("fp32", "bf16", "mixed"):
            E.shape_walk(g, N, H, W, prec)
            for name, d, dd in E.iter_conv_descs(g, N, H, W, prec):
                tag = (gname, prec, name)
                assert lib.mc_conv_tiles(C.byref(d)) > 0, tag
                nbytes = lib.mc_packed_weight_bytes(C.byref(d), 0)
                ext = lib.mc_conv_bank_read_extent(C.byref(d))
                assert nbytes > 0 and 0 < ext <= nbytes, (tag, "forward", ext, nbytes)
                assert lib.mc_wgrad_partial_bytes(C.byref(d)) > 0, tag
                if dd is not None:
                    assert lib.mc_conv_tiles(C.byref(dd)) > 0, tag
                    nb1 = lib.mc_packed_weight_bytes(C.byref(d), 1)
                    ext1 = lib.mc_conv_bank_read_extent(C.byref(dd))
                    assert nb1 > 0 and 0 < ext1 <= nb1, (tag, "input gradient", ext1, nb1)
                checked += 1
    assert checked > 500, checked


@pytest.mark.parametrize("r_p", MODES)
def test_unet6_materialises_exactly_the_unaligned_concats(r_p):
    """Learned padding materialises every two-operand concat; fixed padding only those whose first operand does not fill
    whole channel blocks (the two-source conv kernels keep their c_in0 % 8 == 0 rule)."""
    from pbml_mantle_convection_amd import engine as E
    g = E.unet_graph(5, 10, 6, 2, act="gelu", r_p=r_p, use_symm=False, repeats=3, f=5)
    cats = [[g.channels[s] for s in n.srcs] for n in g.nodes if n.kind == "cat"]
    two = [[g.channels[s] for s in n.srcs] for n in g.nodes if n.kind == "conv" and len(n.srcs) > 1]
    if r_p == "learned":
        assert cats == [[24, 48], [12, 24], [6, 12], [6, 6]] and two == []
    else:
        assert cats == [[12, 24], [6, 12], [6, 6]] and two == [[24, 48]]
    for n in g.nodes:
        if n.kind == "conv" and len(n.srcs) > 1:
            assert g.channels[n.srcs[0]] % 8 == 0


def test_aligned_graphs_keep_their_node_lists():
    """CFG-3's Unet has no CatNode (its concats are the two-source convs); at c_h = 8 / 16 the materialised concats are
    exactly the learned-padding ones, as before."""
    from pbml_mantle_convection_amd import engine as E
    g = E.unet_graph(5, 10, 16, 4, act="gelu", r_p="reflect", use_symm=True, repeats=3, f=5)
    assert not any(n.kind == "cat" for n in g.nodes)
    assert sum(1 for n in g.nodes if n.kind == "conv" and len(n.srcs) == 2) == 4
    for r_p in ("zeros", "replicate"):
        g = E.unet_graph(3, 10, 8, 4, act="gelu", r_p=r_p, use_symm=True, repeats=2, f=5)
        assert not any(n.kind == "cat" for n in g.nodes)
    g = E.unet_graph(3, 10, 8, 4, act="gelu", r_p="learned", use_symm=True, repeats=2, f=5)
    assert [[g.channels[s] for s in n.srcs] for n in g.nodes if n.kind == "cat"] == [[8, 16], [8, 8]]


@pytest.mark.parametrize("r_p", MODES)
def test_plan_gathers_the_gradient_of_unaligned_operands(r_p):
    """Engine.configure (host allocations only): every concat operand that is not exactly its own channel blocks gets a
    gradient buffer of its own, allocated in the plan; the aligned ones read a slice in place.  GroupNorm layers with 6
    channels per group never take the one-launch (power-of-two) paths."""
    from pbml_mantle_convection_amd import engine as E
    g = E.unet_graph(5, 10, 6, 2, act="gelu", r_p=r_p, use_symm=False, repeats=3, f=5)
    for prec in ("fp32", "mixed"):
        e = E.Engine(g, prec)
        e.configure(2, 128, 506, torch.device("cpu"))
        for p in e.plan:
            node = p.node
            if node.kind == "cat":
                off, want = 0, {}
                for k, t in enumerate(node.srcs):
                    c = g.channels[t]
                    if off % 8 or (k < len(node.srcs) - 1 and c % 8):
                        want[t] = off
                    off += c
                assert {t: v[0] for t, v in p.gather.items()} == want
                for t, (_, buf) in p.gather.items():
                    T = e.T[t]
                    assert tuple(buf.shape) == (2, (T.C + 7) // 8, T.H, T.W, 8) and buf.dtype == e.g_dtype
            elif node.kind == "conv" and node.post == 2 and node.gn_name:
                if node.c_out // node.groups not in (1, 2, 4, 8):
                    r = p.route
                    assert r.gn_fwd is not E.GnFwd.SMALL and r.gn_bwd is not E.GnBwd.SMALL and not r.dz_n, node.name
                    assert getattr(p, "pc", None) is None and getattr(p, "dz_pc", None) is None, node.name
        if r_p == "learned":
            assert [len(p.gather) for p in e.plan if p.node.kind == "cat"] == [0, 2, 2, 2]


def test_fluid_trunk_accepts_any_width():
    from pbml_mantle_convection_amd import engine as E
    for c_h in (6, 12, 20):
        for fn in (E.newfluidnet_graph, E.fluidnet_graph):
            g = fn(2, 7, c_h, 1, act="gelu", r_p="learned", use_symm=False, repeats=1, f=5)
            assert [[g.channels[s] for s in n.srcs] for n in g.nodes if n.kind == "cat"] == [[c_h, c_h, 7]]
            E.shape_walk(g, 2, 128, 506, "bf16")


@pytest.mark.parametrize("tag", ["unet6_learned", "unet6_replicate", "newfluidnet12_learned"])
def test_modules_match_reference_state_dict(golden, tag):
    """The c_h = 6 Unet and the c_h = 12 NewFluidNet build with the reference's state_dict keys and shapes."""
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet, Unet
    g = golden(f"g23_{tag}")
    levels, c_i, c_h, c_o, repeats, f, p_pred, symm = [int(v) for v in g["cfg"]]
    if tag.startswith("unet"):
        m = Unet(levels, c_i, c_h, c_o, None, "gelu", str(g["r_p"]), "curl", use_symm=bool(symm), repeats=repeats, f=f,
                 p_pred=bool(p_pred))
    else:
        m = NewFluidNet(levels, c_i, c_h, c_o, None, "gelu", "learned", "curl", use_symm=bool(symm), repeats=repeats, f=f,
                        p_pred=bool(p_pred))
    ref = {n[3:]: g[n].shape for n in g.files if n.startswith("sd/")}
    assert list(m.state_dict().keys()) == list(ref)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == ref
    m.load_state_dict({n[3:]: torch.from_numpy(g[n]) for n in g.files if n.startswith("sd/")}, strict=True)


def test_public_constructors_and_cli_model_factory():
    from pbml_mantle_convection_amd.multigpu import build_model
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet, NewFluidNet, Unet
    for r_p in MODES:
        Unet(5, 10, 6, 2, None, "gelu", r_p, "curl", use_symm=False, repeats=3, f=5)
    for c_h in (6, 12):
        NewFluidNet(2, 7, c_h, 1, None, "gelu", "learned", "curl", repeats=1, f=5, p_pred=False)
        FluidNet(2, 7, c_h, 1, None, "gelu", "learned", "curl", repeats=1, f=5, p_pred=False)
    m = build_model("unet", 5, 10, 6, 2, torch.device("cpu"), "gelu", "learned", "curl", False, 3, 5, a_bound=10)
    assert isinstance(m, Unet)


def test_fluid_trunk_with_fixed_padding_keeps_its_width_rule():
    """The FluidNet-family trunk takes any c_h with learned padding only; with fixed padding an unaligned c_h still fails
    loudly at construction."""
    from pbml_mantle_convection_amd import engine as E
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet, NewFluidNet
    for r_p in ("zeros", "reflect", "replicate"):
        for fn in (E.newfluidnet_graph, E.fluidnet_graph):
            with pytest.raises(NotImplementedError, match="multiple of 8"):
                fn(2, 7, 12, 1, act="gelu", r_p=r_p, use_symm=False, repeats=1, f=5)
            fn(2, 7, 16, 1, act="gelu", r_p=r_p, use_symm=False, repeats=1, f=5)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        NewFluidNet(2, 7, 6, 1, None, "gelu", "zeros", "curl", repeats=1, f=5, p_pred=False)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        FluidNet(2, 7, 6, 1, None, "gelu", "replicate", "curl", repeats=1, f=5, p_pred=False)


def test_symmetric_filters_at_width_6_fail_loudly():
    """use_symm at c_h = 6 (not in the run list) is refused by the convolution descriptors, before any launch."""
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import engine as E
    g = E.unet_graph(3, 10, 6, 2, act="gelu", r_p="replicate", use_symm=True, repeats=2, f=5)
    with pytest.raises(L.MantleHipError, match="unsupported convolution configuration"):
        E.Engine(g, "fp32").configure(2, 40, 54, torch.device("cpu"))


def test_cat_grad_gather_is_declared_and_validates_before_launch():
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    assert hasattr(lib, "mc_cat_grad_gather") and "mc_cat_grad_gather" in L.SIGNATURES
    EINVAL, EUNSUP = -1, -2
    fake = C.c_void_p(0x1000)
    g = L.GradSrc(0x1000, L.GSRC_PLAIN, 0, 0, 1, 8, 10)

    def rc(gs, c_total=12, c_off=6, c=6, n=2, h=8, w=10, dtype=L.MC_F32, out=fake):
        return lib.mc_cat_grad_gather(C.byref(gs) if gs is not None else None, c_total, c_off, c, n, h, w, dtype, out, None)
    assert rc(None) == EINVAL
    assert rc(g, out=None) == EINVAL
    assert rc(g, c_off=7) == EINVAL                                   # past the concatenated tensor's channels
    assert rc(g, c=0) == EINVAL and rc(g, c_off=-1) == EINVAL and rc(g, n=0) == EINVAL
    assert rc(g, h=9) == EINVAL                                       # the source must cover the operand's H x W
    assert rc(L.GradSrc(0x1000, L.GSRC_PLAIN, 0, 0, 1, 8, 10, 2, 1)) == EINVAL     # a slice is not a whole tensor
    assert rc(L.GradSrc(0x1000, L.GSRC_PADFOLD_POOL, 1, 0, 2, 8, 10)) == EUNSUP
    assert rc(L.GradSrc(0x1000, L.GSRC_PADFOLD, 3, 0, 1, 8, 10)) == EUNSUP      # (pad > 2: check_gsrc)
    assert rc(g, dtype=99) == EUNSUP
    assert L.load().mc_strerror(EUNSUP) == b"unsupported configuration"

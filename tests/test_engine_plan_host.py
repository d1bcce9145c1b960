"""The engine's host side -- which launches run, with which buffers -- without a device: the routes Engine.configure decides
for the headline U-Net and under every switch, the launches of one forward + backward (tests/engine_trace.py) against those
routes, and that a step leaves nothing behind in the plan.  No GPU."""
import copy
import functools
from collections import Counter

import pytest
import torch

import engine_trace as ET

PRECISIONS = ET.PRECISIONS
# input-gradient launches of the headline U-Net that carry their producer's GroupNorm-backward reduction ("mixed")
EPILOGUES = {"conv.1.layers.0.", "conv.2.layers.0.", "convs.0.1.layers.0.", "convs.0.2.layers.0.", "upconvs.2.1.layers.0.",
             "upconvs.2.2.layers.0.", "conv.4.", "conv.5."}
LAYER_SHAPE = (2, 64, 96)


def _E():
    return ET._modules()[1]


@functools.lru_cache(maxsize=None)
def _graph(name):
    E, kw = _E(), dict(act="gelu", use_symm=True, f=5)
    if name == "unet":
        return ET.headline()
    if name == "convae":
        return E.convae_graph(2, 3, 16, 3, act="gelu", r_p="reflect", use_symm=True, repeats=2, f=3, loss_type="mae")
    if name == "unet learned":
        return E.unet_graph(3, 10, 8, 4, r_p="learned", repeats=2, **kw)
    return E.newfluidnet_graph(3, 7, 16, 4, r_p="reflect", repeats=2, drop_rate=0.25 if name == "net drop" else 0.0, **kw)


SHAPES = {"unet": ET.HEADLINE, "convae": (2, 64, 48), "unet learned": (2, 48, 70), "net drop": LAYER_SHAPE, "net": LAYER_SHAPE}
FUSE3 = tuple(ET.FUSE3.items())
# (graph, precision, switches): every row whose routes are asserted below, and which the trace is checked against
ROWS = ([("unet", p, ()) for p in PRECISIONS] + [("unet", p, FUSE3) for p in PRECISIONS]
        + [("unet", "mixed", tuple(ET.SWITCHES[s].items())) for s in ("dz_rr0", "wgrad_dz0", "gn_small0")]
        + [(g, p, FUSE3) for g in ("net drop", "net") for p in PRECISIONS]
        + [("convae", "fp32", ()), ("unet learned", "mixed", ()), ("net drop", "mixed", ())])


@functools.lru_cache(maxsize=None)
def _run(graph, precision, env=()):
    """(engine, forward + backward entries of its first step, of its second step, plan and tensor records before the steps)."""
    eng = ET.make_engine(_graph(graph), precision, dict(env))
    eng.configure(*SHAPES[graph], torch.device("cpu"))
    before = [copy.copy(e) for e in eng.plan], {k: copy.copy(t) for k, t in eng.T.items()}
    (f1, b1), (f2, b2) = ET.trace_step(eng, SHAPES[graph], drop=graph == "net drop", steps=2)
    return eng, f1 + b1, f2 + b2, before


def _layers(eng):
    return [e for e in eng.plan if e.node.kind == "conv"]


def _epilogues(eng):
    return {e.node.name for e in eng.convs if e.route.epi >= 0}


def _count(eng, what):
    return sum(1 for e in _layers(eng) if what(e))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_headline_routes(prec):
    E = _E()
    eng = _run("unet", prec)[0]
    layers = _layers(eng)
    assert len(layers) == 27 and len(eng.plan) == len(eng.g.nodes) and all(e.node is n for e, n in zip(eng.plan, eng.g.nodes))
    assert _count(eng, lambda e: e.node.post == E.L.POST_GN_ACT) == 25
    assert _count(eng, lambda e: e.route.gn_fwd is E.GnFwd.SMALL) == 15
    assert _count(eng, lambda e: e.route.gn_bwd is E.GnBwd.SMALL) == 15
    assert [e.route.bwd for e in eng.plan if e.op == "up"] == [E.UpBwd.WALK] * 4
    assert not any(t.fused for t in eng.T.values())
    if prec != "mixed":
        assert _epilogues(eng) == set() and not _count(eng, lambda e: e.route.gn_bwd in E.DZ_ROUTES)
        return
    assert _epilogues(eng) == EPILOGUES
    assert {eng.plan[e.route.epi].node.out for e in eng.convs if e.route.epi >= 0} == \
        {e.node.out for e in layers if e.route.gn_bwd in E.DZ_ROUTES}
    assert _count(eng, lambda e: e.route.gn_bwd is E.GnBwd.DZ_WGRAD) == 5
    assert _count(eng, lambda e: e.route.dz_n) == 3
    small = (E.GnFwd.SMALL, E.GnBwd.SMALL)
    assert not _count(eng, lambda e: e.route.gn_bwd in E.DZ_ROUTES and (e.route.gn_fwd in small or e.route.gn_bwd in small))


def test_convae_upsamples_take_the_separable_adjoint():
    E = _E()
    eng = _run("convae", "fp32")[0]
    ups = [e for e in eng.plan if e.op == "up"]
    assert [e.route.bwd for e in ups] == [E.UpBwd.SEPARABLE] * 2 and all(e.bws is not None for e in ups)


def test_switches_mixed():
    E = _E()

    def eng(name):
        return _run("unet", "mixed", tuple(ET.SWITCHES[name].items()))[0]
    assert _epilogues(eng("dz_rr0")) == set()
    e = eng("wgrad_dz0")
    assert _epilogues(e) == EPILOGUES and not _count(e, lambda p: p.route.gn_bwd is E.GnBwd.DZ_WGRAD)
    assert _count(e, lambda p: p.route.gn_bwd is E.GnBwd.DZ_APPLY) == 8
    e = eng("gn_small0")
    assert not _count(e, lambda p: p.route.gn_fwd is E.GnFwd.SMALL or p.route.gn_bwd is E.GnBwd.SMALL)
    assert e.sw.gn_small_pix == 0 and eng("dz_rr0").sw.fuse_dz_rr is False and eng("wgrad_dz0").sw.wgrad_dz is False


@pytest.mark.parametrize("prec", PRECISIONS)
def test_fuse_everything_fuses_and_spares_the_dropout_nodes(prec):
    """MANTLE_FUSE=3 without a pixel limit: fused tensors and dz epilogues in every precision; on a dropout graph none on the
    dropout nodes (what test_dropout_nodes_are_materialised_and_keep_their_own_backward asserts on the device)."""
    E = _E()
    eng = _run("unet", prec, FUSE3)[0]
    assert eng.fuse == 3 and any(t.fused for t in eng.T.values()) and _epilogues(eng)
    found = {}
    for name in ("net drop", "net"):
        eng = _run(name, prec, FUSE3)[0]
        trunk = [e for e in _layers(eng) if e.node.name.startswith(("conv.0.", "convs."))]
        assert len(trunk) == 7 and all((e.node.drop > 0) == (name == "net drop") for e in trunk)
        found[name] = [(e.route.fused, eng.T[e.node.out].fused, e.route.gn_bwd in E.DZ_ROUTES,
                        any(o.route.epi >= 0 and eng.plan[o.route.epi] is e for o in eng.convs)) for e in trunk]
    assert not any(any(t) for t in found["net drop"]), found["net drop"]
    assert any(any(t) for t in found["net"]), "the twin fuses nothing: the check above shows nothing"


def _expected(eng, drop):
    """Entry name -> number of launches one forward + backward must issue, read off the plan's routes."""
    E = _E()
    c = Counter()
    for e in eng.plan:
        if e.op == "up":
            c["mc_bicubic_bwd_" + e.route.bwd.value] += 1
        if e.node.kind != "conv":
            continue
        r, gn, sfx = e.route, e.node.post == E.L.POST_GN_ACT, "_drop" if drop and e.node.drop > 0 else ""
        if r.gn_fwd is E.GnFwd.SMALL:
            c["mc_gn_act_fwd_small" + sfx] += 1
        elif r.gn_fwd is E.GnFwd.MEANS:
            c["mc_gn_finalize"] += 1
        elif r.gn_fwd in (E.GnFwd.APPLY, E.GnFwd.FUSED):
            c["mc_gn_finalize_coef"] += gn
            c["mc_gn_act_fwd" + sfx] += r.gn_fwd is E.GnFwd.APPLY or e.node.pool > 1
        if r.gn_bwd is E.GnBwd.SMALL:
            c["mc_gn_act_bwd_small" + sfx] += 1
        elif r.gn_bwd is E.GnBwd.APPLY:
            c["mc_gn_act_bwd_reduce" + sfx] += gn
            c["mc_gn_act_bwd_finalize"] += gn
            c["mc_gn_act_bwd_apply" + sfx] += 1
        elif r.gn_bwd in E.DZ_ROUTES:
            wdz = r.gn_bwd is E.GnBwd.DZ_WGRAD
            c["mc_gn_act_bwd_finalize" + ("_n" if r.dz_n else "") + ("_dz" if wdz else "")] += gn
            c["mc_conv2d_wgrad_dz" if wdz else "mc_gn_bwd_apply_dz"] += 1
        if e.op == "conv":
            c["mc_conv2d_wgrad_fused"] += r.gn_bwd is not E.GnBwd.DZ_WGRAD
            c["mc_fold_padded_dz"] += e.route.epi >= 0
    return +c


ROUTED = ("mc_bicubic_bwd_", "mc_gn_", "mc_conv2d_wgrad_fused", "mc_conv2d_wgrad_dz", "mc_fold_padded_dz")
NOT_ROUTED = ("mc_gn_partials", "mc_gn_param_grads_batched")
# pointer arguments a routed launch cannot do without, by position ("_drop" entries: as their plain twins); a struct is named
# with the fields that must be set
REQUIRED = {
    "mc_gn_act_fwd_small": (0, 1, 9, 10, 14, 15), "mc_gn_finalize_coef": (0, 7, 8, 9), "mc_gn_finalize": (0, 8), "mc_gn_act_fwd": (0,),
    "mc_gn_act_bwd_small": (0, 6, 7, 8, (11, "ptr"), 13, 14), "mc_gn_act_bwd_reduce": (0, 6, 7, 8, (12, "ptr"), 14),
    "mc_gn_act_bwd_finalize": (0, 6, 7, 8, 9), "mc_gn_act_bwd_finalize_dz": (0, 6, 7, 8, 9, 10, 11),
    "mc_gn_act_bwd_finalize_n": (0, 6, 7, 8), "mc_gn_act_bwd_finalize_n_dz": (0, 6, 7, 8, 9, 10),
    "mc_gn_act_bwd_apply": (0, (13, "ptr"), 15), "mc_gn_bwd_apply_dz": ((0, "ptr"), 1, 10),
    "mc_conv2d_wgrad_dz": (1, (3, "ptr"), 4, 5, 6, 7), "mc_conv2d_wgrad_fused": (1, 4, 5), "mc_fold_padded_dz": (0, 8, 11),
    "mc_bicubic_bwd_walk": ((0, "ptr"), 7, 8, 9, 10, 11, 12, 13, 16), "mc_bicubic_bwd_separable": ((0, "ptr"), 14, 15),
    "mc_bicubic_bwd_taps": ((0, "ptr"), 16)}


@pytest.mark.parametrize("graph, prec, env", ROWS, ids=lambda v: v if isinstance(v, str) else "+".join(k[7:] for k, _ in v) or "default")
def test_trace_issues_the_launches_the_routes_name(graph, prec, env):
    """The launches of a step are the ones the routes name, and no pointer such a launch needs is NULL.  The limit of this
    check: it does not know WHICH buffer belongs in a place -- e.gpart passed where e.m12 belongs passes it.  That a launch
    receives the right buffers rests on comparing the whole traces (`python tests/engine_trace.py OUT.json`) of a change to
    the engine with those of its parent commit, and on the bit-identity tests of the GPU suite."""
    E = _E()
    eng, trace, _, _ = _run(graph, prec, env)
    got = Counter(n for n, _ in trace if n.startswith(ROUTED) and n not in NOT_ROUTED)
    assert got == _expected(eng, drop=graph == "net drop")
    epilogues = 0
    for name, args in trace:
        plain = name[:-5] if name.endswith("_drop") else name
        for pos in REQUIRED.get(plain, ()):
            pos, field = pos if isinstance(pos, tuple) else (pos, None)
            assert (args[pos] if field is None else args[pos][field]) is not None, (name, pos, args)
        if plain == "mc_gn_act_fwd":
            assert args[13] is not None or args[14] is not None, (name, args)
        for entry, post, idx in (("mc_gn_act_fwd", 9, (6, 7, 8)), ("mc_gn_act_bwd_apply", 10, (6, 7, 8, 9))):
            if plain == entry and args[post] == E.L.POST_GN_ACT:         # a GroupNorm layer: statistics and affine too
                assert all(args[i] is not None for i in idx), (name, args)
        if name == "mc_conv2d_fused" and args[9] is not None:
            epilogues += 1
            assert args[9]["y"] is not None and args[9]["partials"] is not None and args[9]["part_stride"] > 0, args
    assert epilogues == len(_epilogues(eng))
    if graph == "net drop":
        assert trace[0][0] == "mc_dropout_advance" and any(n.endswith("_drop") for n, _ in trace)


@pytest.mark.parametrize("graph, prec, env", [r for r in ROWS if r[2] in ((), FUSE3)],
                         ids=lambda v: v if isinstance(v, str) else "+".join(k[7:] for k, _ in v) or "default")
def test_a_step_leaves_nothing_in_the_plan(graph, prec, env):
    eng, first, second, (plan, T) = _run(graph, prec, env)
    assert first == second and len(first) > 10
    assert plan == eng.plan and T == eng.T
    assert all(type(a) is type(b) for a, b in zip(plan, eng.plan))


def test_a_misspelt_field_is_an_error():
    eng = _run("unet", "fp32")[0]
    for e in eng.plan:
        with pytest.raises(AttributeError):
            e.dz_cof = None
    with pytest.raises(AttributeError):
        eng.plan[0].route.gn_fwd = None

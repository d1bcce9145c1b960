"""The loss's host side -- which launches run, with which planes -- without a device: the plan `StokesLoss` chooses in its
constructor for every row of tests/loss_trace.py, the launches of two evaluations against that plan, the zeroing rule, the
plane pointers against the channel map, `unplanned_copy`, and the three autograd functions of the curl heads.  No GPU."""
import functools
import os

import pytest

import loss_trace as LT

ROWS = LT.table()
MOM = {"yc", "paras", "scaler"}
# positions of (u, v, T, p) among the arguments of the loss launches, for the source planes and for the gradient planes
FWD_BWD = dict(src=(1, 2, 4, 3), grad=(10, 11, 13, 12))
FUSED = dict(src=(1, 2, 4, 3), grad=(18, 19, 21, 20))


def _mods():
    losses = LT._losses()
    from pbml_mantle_convection_amd import heads
    return losses, heads


@functools.lru_cache(maxsize=None)
def _run(name):
    """(loss, Cc, trace) of a row."""
    row = ROWS[name]
    with LT.fused_loss(row["fused"]):
        loss, Cc = LT.build(row)
        return loss, Cc, LT.trace_loss(loss, LT.N, Cc, LT.H, LT.W, cb8=row["cb8"])


def _expected_plan(row):
    """(route, head form, (u, v, T, p), ct, zero, needs) by the rules of DESIGN.md §1 "The loss's plan and routes"."""
    kw = row["kw"]
    has_T, p_pred, curl = kw.get("has_T", True), kw["p_pred"], kw["loss_type"] == "curl"
    needs = (MOM if kw.get("lambda_mom") else set()) | ({"advect", "scaler"} if kw.get("advect_cn") else set())
    ct = 2 + int(p_pred) + int(has_T)
    if curl:
        form = "VALID" if kw.get("curl_valid") else "WALL_T" if has_T else "WALL"
        chans = ("head", "head", "head" if has_T else None, (1 + int(has_T)) if p_pred else None)
        return "SPLIT", form, chans, ct, "EXTRA_CHANNELS_ONLY" if form == "VALID" else "ALWAYS", needs
    route = "FUSED" if has_T and row["fused"] is not False else "SPLIT"
    return route, None, (0, 1, 2 if has_T else None, (2 + int(has_T)) if p_pred else None), ct, "EXTRA_CHANNELS_ONLY", needs


def _plan_launches(loss):
    losses, heads = _mods()
    plan = loss.plan
    fwd, bwd = heads.ENTRIES[plan.head.form, plan.head.blurr] if plan.head is not None else (None, None)
    if plan.route is losses.LossRoute.FUSED:
        names = ["mc_loss_fused"]
    else:
        names = [fwd, "mc_loss_fwd_bwd"]
        names += ["mc_advect_loss_dt", "mc_advect_loss"] if "advect" in plan.needs else []
        names += ["mc_momentum_residual", "mc_momentum_adjoint"] if "yc" in plan.needs else []
        names += [bwd]
    return (["mc_loss_minmax"] if loss.loss_scale else []) + [n for n in names if n] + ["mc_loss_finalize"]


@pytest.mark.parametrize("name", list(ROWS))
def test_plan_fields(name):
    losses, heads = _mods()
    loss, row = _run(name)[0], ROWS[name]
    route, form, chans, ct, zero, needs = _expected_plan(row)
    plan = loss.plan
    assert plan.route is losses.LossRoute[route] and loss.fusable() == (route == "FUSED")
    assert (plan.head.form.name if plan.head is not None else None) == form
    if plan.head is not None:
        assert plan.head.blurr == bool(row["kw"].get("blurr")) and plan.head.a_bound == loss.a_bound
    assert plan.chan == tuple(losses.HEAD if c == "head" else c for c in chans)
    assert plan.ct == ct and plan.zero is losses.Zero[zero]
    assert plan.needs == frozenset(needs) and loss.needs is plan.needs
    with pytest.raises(AttributeError):
        plan.route = losses.LossRoute.SPLIT


@pytest.mark.parametrize("name", list(ROWS))
def test_trace_issues_the_plans_launches(name):
    losses, _ = _mods()
    loss, Cc, tr = _run(name)
    assert [e[0] for e in tr["first"]] == _plan_launches(loss)
    # nothing is allocated or decided again on the second call
    assert tr["second"][:-2] == tr["first"]
    zeroed = loss.plan.zero is losses.Zero.ALWAYS or Cc > loss.channels_needed()
    assert tr["second"][-2:] == [("gy.zero_", [zeroed]), ("sums.zero_", [True])]


@pytest.mark.parametrize("name", list(ROWS))
def test_plane_pointers_follow_the_channel_map(name):
    losses, heads = _mods()
    loss, Cc, tr = _run(name)
    plan, lab, calls = loss.plan, tr["labels"], dict(tr["first"])
    fused = plan.route is losses.LossRoute.FUSED
    args, pos = (calls["mc_loss_fused"], FUSED) if fused else (calls["mc_loss_fwd_bwd"], FWD_BWD)
    fwd, bwd = (calls[n] for n in heads.ENTRIES[plan.head.form, plan.head.blurr]) if plan.head is not None else (None, None)
    valid = plan.head is not None and plan.head.form is heads.HeadForm.VALID
    head_out = dict(zip("uvT", fwd[6:8] + [None] if valid else fwd[9:12])) if fwd else {}
    head_in = dict(zip("uvT", bwd[0:2] + [None] if valid else bwd[0:3])) if bwd else {}
    for i, (term, c) in enumerate(zip("uvTp", plan.chan)):
        src, grad = args[pos["src"][i]], args[pos["grad"][i]]
        if c is None:
            assert src is None and grad is None, term
        elif c is losses.HEAD:
            assert src is not None and src == head_out[term] and grad is not None and grad == head_in[term], term
            assert src not in lab.values() and grad not in lab.values(), term
        else:
            assert grad is not None and grad == lab[f"gy+{c}"], term
            # (the CB8 form reads no plane of y)
            assert src is None if ROWS[name]["cb8"] else (src is not None and src == lab[f"y+{c}"]), term
    if plan.head is not None:
        y0, g0 = (fwd[0], bwd[6]) if valid else (fwd[0], bwd[10])
        assert y0 == lab["y+0"] and g0 == lab["gy+0"] and y0 is not None and g0 is not None
        if plan.head.form is heads.HeadForm.WALL_T:              # T = channel 1: read by the clip, forward and backward
            assert fwd[1] == bwd[3] == lab["y+1"] and bwd[11] == lab["gy+1"] and None not in (fwd[1], bwd[11])
        elif not valid:
            assert fwd[1] is None and fwd[11] is None and bwd[2] is None and bwd[3] is None and bwd[11] is None


@pytest.mark.parametrize("name", ["unet mass p1 lam1e-06 split", "unet mass p1 lam1e-06 cb8", "unet curl p1 lam1e-06",
                                  "fluidnet ad1 blurr1"])
def test_unplanned_copy(name):
    row = ROWS[name]
    with LT.fused_loss(row["fused"]):
        loss, Cc = LT.build(row)
        LT.trace_loss(loss, LT.N, Cc, LT.H, LT.W, cb8=row["cb8"])
        loss.freeze()
    # (outside the block FUSED_LOSS is back at its default: the copy carries the plan, it does not decide again)
    lo = loss.unplanned_copy()
    assert lo.plan is loss.plan and lo._shape is None and not lo._frozen and loss._frozen
    assert lo.gradient_sums() is None and not any(hasattr(lo, b) for b in ("gy", "sums", "out8", "mm", "cu", "sx", "adv_dt"))
    assert LT.trace_loss(lo, LT.N, Cc, LT.H, LT.W, cb8=row["cb8"]) == _run(name)[2]
    assert lo.gy is not loss.gy
    args, kw = LT.loss_inputs(loss, LT.N + 1, Cc, LT.H, LT.W, row["cb8"])
    with LT.ET.host_stubs(), pytest.raises(RuntimeError, match="pinned to shape"):
        loss.evaluate(*args, **kw)


@pytest.mark.parametrize("name", list(LT.head_table()))
def test_autograd_functions_launch_through_the_head_table(name):
    _, heads = _mods()
    fn, shape, blurr = LT.head_table()[name]
    form = {"_CurlHead": heads.HeadForm.WALL_T, "_CurlUV": heads.HeadForm.WALL, "_CurlValid": heads.HeadForm.VALID}[fn]
    (f, fa), (b, ba) = LT.trace_head(fn, shape, blurr)
    assert (f, b) == heads.ENTRIES[form, bool(blurr)]
    n, c, hy, wy = shape
    h, w = heads.CurlHead(form, bool(blurr)).out_hw(hy, wy)
    if form is heads.HeadForm.VALID:
        assert fa[:6] == [1, n, h, w, c * hy * wy, 10.0] and ba[2:6] == [n, h, w, 10.0] and ba[7] == c * hy * wy
    else:
        clip = [10.0, 0.0, 1.5] if form is heads.HeadForm.WALL_T else [10.0, 0.0, 0.0]
        assert fa[2:9] == [n, h, w, c * h * w] + clip and ba[4:10] == [n, h, w] + clip and ba[12:14] == [c * h * w] * 2
        assert (fa[1] is None) == (form is heads.HeadForm.WALL) and fa[1] == ba[3]


def test_head_refuses_a_blurred_unet():
    _, heads = _mods()
    with pytest.raises(ValueError, match="blurr is the streamfunction blur of NewFluidNet / FluidNet"):
        heads.CurlHead(heads.HeadForm.WALL_T, True)
    with pytest.raises(ValueError, match="blurr is the streamfunction blur of NewFluidNet / FluidNet"):
        LT._losses().StokesLoss(True, "curl", blurr=True)


def test_head_launches_are_named_in_one_place():
    losses, _ = _mods()
    pkg = os.path.dirname(os.path.abspath(losses.__file__))
    for mod in ("losses.py", "multigpu.py"):
        with open(os.path.join(pkg, mod)) as f:
            assert "mc_curl_" not in f.read(), mod

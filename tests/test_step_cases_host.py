"""CPU-only checks of tests/step_cases.py, the harness of tests/test_hip_step_kernels.py: the f64 restatements equal the oracle
(adnet_step, the input channels of ts_rollout / ts_rollout_unet, the channel-6 rule of unet_roll_forward, the g18 / g19 items); the
conditions on the inputs hold for every case; every mutant of the references fails the comparison functions the GPU tests use, and
the mutants only the stretched grid can catch pass on the uniform one; the existing gate on mc_adnet_step passes a step without
its heating term."""
import numpy as np
import pytest
import torch

import fields
import loss_cases as Lc
import step_cases as Sc
from oracle import ref_cpu as O
from test_dataset_shards import _write_tree

f64 = torch.float64
ALL_STEP = [(N, H, W, g) for N, H, W in Sc.STEP_SHAPES + [Sc.STEP_BIG] for g in (False, True)]
In = (slice(None), slice(1, -1), slice(1, -1))


def _good(c, dt, s=None, raq=None, **mut):
    return Sc.stored(Sc.t64(Sc.step64(c, dt, s, raq, **mut))).numpy()


# ---- the restatements -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W,g", [(3, 5, 6, False), (3, 5, 6, True), (2, 9, 70, True), (1, 3, 3, True)])
def test_step_restatement_equals_the_oracle(N, H, W, g):
    c = Sc.step_case(N, H, W, g)
    for s in (None, c["vs"]):
        sc = np.ones(N) if s is None else s
        inp = np.stack([c["u"] * sc[:, None, None], c["v"] * sc[:, None, None], c["T"], c["raq_field"],
                        np.broadcast_to(c["xc"], (N, H, W)), np.broadcast_to(c["yc"], (N, H, W))], 1)
        cn = float(np.float32(Sc.CN))
        Tn, dt = O.adnet_step(torch.from_numpy(inp.astype(np.float64)), CN_max=cn)
        assert abs(float(dt) - Sc.dt64(c, s)) <= 1e-13 * float(dt)
        mine = Sc.step64(c, float(dt), s, c["raq_field"])
        assert np.abs(mine - Tn[:, 0].numpy()).max() <= 1e-13
        Tn2, _ = O.adnet_step(torch.from_numpy(inp.astype(np.float64)), dt=torch.tensor(1e-5, dtype=f64))
        assert np.abs(Sc.step64(c, 1e-5, s, c["raq_field"]) - Tn2[:, 0].numpy()).max() <= 1e-13


def _close(a, b, atol=2e-9):
    """(the oracle clips at the double 1e-8, the kernels and this reference at f32(1e-8): 3e-10 in the channel)"""
    assert float((a - b).abs().max()) <= atol, float((a - b).abs().max())


@pytest.mark.parametrize("N,H,W", [(3, 5, 6), (2, 33, 130)])
def test_builder_restatements_equal_the_oracle(N, H, W):
    c = Sc.build_case(N, H, W)
    v4 = lambda t: t.reshape(1, 1, H, W)  # noqa: E731
    for unet in (False, True):
        chans = Sc.build_input_ref(c, unet)
        for n in range(N):
            seen = []

            def stokes(inp):
                seen.append(inp.clone())
                z = torch.zeros((1, 1, H, W), dtype=f64)
                return (z, z, None, v4(c["Tn"][n])) if unet else (z, z, None)
            raq, fkt, fkp = c["paras"][n]
            nd = c["nd"][n]
            if unet:
                O.ts_rollout_unet(stokes, v4(c["T"][n]), v4(c["ycc"]), nd[0], nd[1], nd[2], fkt, fkp, v4(c["xc"]), v4(c["yc"]),
                                  v4(c["up"][n]), v4(c["vp"][n]), v4(c["dt"][n]), ts=1)
            else:
                O.ts_rollout(stokes, v4(c["T"][n]), v4(c["ycc"]), nd[0], nd[1], nd[2], raq, fkt, fkp, v4(c["xc"]), v4(c["yc"]), ts=1)
            for k, (_, ref, _) in enumerate(chans):
                _close(seen[0][0, k], ref[n])
    # the channel-6 rule of the roll-forward chain: rewritten after a pre-step, left alone after a round's last step
    x0 = Sc.roll_x0(c, 10)
    seen = []

    def forward(x):
        seen.append(x.clone())
        return c["u"], c["v"], None, c["Tn"]
    O.unet_roll_forward(forward, x0, c["paras"], 2)
    ref1, _ = Sc.roll_forward_ref(c, x0, 1)
    ref0, _ = Sc.roll_forward_ref(c, ref1, 0)
    _close(seen[1][:, 6:10], ref1[:, 6:10])
    _close(seen[2][:, 6:10], ref0[:, 6:10])
    assert torch.equal(seen[2][:, 6], seen[1][:, 6]) and not torch.equal(seen[1][:, 6], seen[0][:, 6])


def _store_of(ds, uv, t):
    """The arrays of a host dataset as the resident classes keep them (f32), in the layout of Sc.store_case."""
    T = torch.stack([x.reshape(x.shape[-2], x.shape[-1]) for x in ds.x_data]).double()
    H, W = T.shape[-2:]
    return dict(m=T.shape[0], H=H, W=W, cy=uv.shape[1], T=Sc.r32(T), uv=Sc.r32(uv), t=Sc.r32(t),
                paras=Sc.r32(torch.stack([p.reshape(3) for p in ds.paras])), nd=Sc.r32(torch.stack([p.reshape(3) for p in ds.paras_nd])),
                xc=Sc.r32(ds.xc.reshape(H, W)), yc=Sc.r32(ds.yc.reshape(H, W)))


def _items_close(chans, want):
    """Within the f32 rounding of the stored inputs and of the one f32 operation (3 U, relative), the viscosity within its bound."""
    for k, (name, ref, tol) in enumerate(chans):
        w = want[k].double()
        assert bool(((ref - w).abs() <= 3 * Sc.U * w.abs() + 2 * tol + 2e-9).all()), name


def test_item_restatements_equal_the_golden_items(golden, tmp_path):
    import random
    from pbml_mantle_convection_amd.datasetio import ADTimeDataset, NewADDataset
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    g = golden("g18_newad_dataset")
    _write_tree(g, str(tmp_path / "a"))
    ds = NewADDataset(str(tmp_path / "a"), scale=True, load=False, noise=0.0, an="train", is_init=False, p_pred=True, debug=False)
    S = _store_of(ds, torch.stack(list(ds.y_data)).double(), torch.stack([t.reshape(()) for t in ds.t_data]).double())
    for i in range(len(ds)):
        x, y, t, s = ds[i]
        np.testing.assert_allclose(x.numpy(), g["all/x"][i], rtol=1e-12, atol=1e-14)       # (the items are the reference's)
        xr, yr, s64, s_tol, tw = Sc.newad_item_ref(S, i)
        _items_close(xr, x)
        _items_close(yr, y)
        assert abs(float(s64) - float(torch.as_tensor(s).reshape(()))) <= 1e-6 * float(s64) and float(tw) == float(np.float32(float(t)))
    g = golden("g19_adtime_dataset")
    _write_tree(g, str(tmp_path / "b"))
    ds = ADTimeDataset(str(tmp_path / "b"), scale=True, load=False, noise=0.0, an="train", p_pred=True, debug=False, roll_forward=1)
    S = _store_of(ds, torch.stack(list(ds.y_data)).double(), torch.tensor([float(v) for v in ds.t], dtype=f64))
    done = 0
    for i in range(len(ds)):
        i0, i1 = ds.indices[i]
        if i0 % 8 == 0:
            continue                                           # (these draw a random pair)
        random.seed(0)
        x, y, s, par, _ = ds[i]
        xr, yr, s64, s_tol, pr = Sc.adtime_item_ref(S, i0, i1)
        # t1 - t0 of two f32-rounded times is off by the rounding of the times, not of the difference
        xr[2] = ("t1-t0", x[2].double(), xr[2][2] + 2 * Sc.U * float(max(abs(S["t"][i0]), abs(S["t"][i1]))))
        _items_close(xr, x)
        _items_close(yr, y)
        assert abs(float(s64) - float(torch.as_tensor(s).reshape(()))) <= 1e-6 * float(s64)
        done += 1
    assert done >= 3


# ---- the conditions on the inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", sorted({(H, W) for _, H, W in Sc.STEP_SHAPES + [Sc.STEP_BIG, (2, 130, 260)]}))
def test_stretched_grid(H, W):
    xc, yc = Sc.grid_stretched(H, W)
    assert np.isnan(xc[:, 0]).all() and np.isnan(xc[:, -1]).all() and np.isnan(yc[0]).all() and np.isnan(yc[-1]).all()
    assert np.isfinite(xc[:, 1:-1]).all() and np.isfinite(yc[1:-1]).all()
    x, y = Sc.with_walls(xc, yc)
    sx, sy = np.diff(x, axis=1), np.diff(y, axis=0)
    assert (sx > 0).all() and (sy > 0).all()                                       # strictly increasing along their axis
    for s, ax in ((sx, 1), (sy, 0)):
        a, b = (s[:, 1:], s[:, :-1]) if ax == 1 else (s[1:], s[:-1])
        assert (np.maximum(a / b, b / a) >= 1.2).all()                             # neighbouring spacings differ by >= 20 %
    if H > 3:
        assert len(set(x[1:-1, 1].tolist())) > 1                                   # sheared: the shift depends on the row
    if W > 3:
        assert len(set(y[1, 1:-1].tolist())) > 1
    xf, yf = Sc.grid_stretched(H, W, finite_walls=True)
    assert np.isfinite(xf).all() and np.isfinite(yf).all() and np.array_equal(xf[:, 1:-1], xc[:, 1:-1])
    assert not np.array_equal(yf, Sc.grid_uniform(H, W)[1])                        # yc and ycc differ


@pytest.mark.parametrize("N,H,W,g", ALL_STEP)
def test_step_case_conditions(N, H, W, g):
    c = Sc.step_case(N, H, W, g)
    P = (H - 2) * (W - 2)
    u, v = c["u"][In], c["v"][In]
    assert (u == 0).reshape(N, -1).any(1).all()
    if P > 1:
        assert (v == 0).reshape(N, -1).any(1).all()
        for f in (u, v):
            assert (f > 0).any() and (f < 0).any()
    if N >= 2:
        assert not c["u"][N - 1].any() and not c["v"][N - 1].any()
    for s in (None, c["vs"]):
        dt = float(Sc.dt32(c, s))
        adv, dif = Sc.increments(c, dt, s)
        print(f"\n{N}x{H}x{W} stretched={g} scaled={s is not None}: dt {dt:.3e} advective {adv:.3e} diffusive {dif:.3e}")
        assert adv > 0 and dif > 0 and max(adv / dif, dif / adv) <= Sc.BALANCE
        # the reference passes its own comparison, and the f32 step lies within its f64 bound
        assert Sc.check_step(c, _good(c, dt, s), dt, s)[0] == []
        assert Sc.check_dt(Sc.dt32(c, s), c, s)[0] == []


def _visc_cases():
    for N, H, W in Sc.BUILD_SHAPES[1:] + [Sc.BUILD_BIG]:
        c = Sc.build_case(N, H, W)
        yield f"builders {N}x{H}x{W}", c["T"], c["ycc"], c["paras"]
        yield f"roll-forward {N}x{H}x{W}", c["Tn"], c["yc"], c["paras"]
    for H, W in Sc.ASM_SHAPES[1:]:
        S = Sc.store_case(H, W, 2)
        yield f"store {H}x{W}", S["T"], S["yc"], S["paras"]


def test_viscosity_cases_hit_both_clips_and_both_seams():
    """(the one-pixel cases cannot: they are left out)"""
    for name, T, y, paras in _visc_cases():
        lo, hi, near_lo, near_hi = Sc.clip_shares(T, y, paras)
        print(f"\n{name}: clipped at 1e-8 {lo:.3f}, at 1 {hi:.3f}; within E_ETA of the seams {near_lo}, {near_hi}")
        assert 0 < lo <= 0.5 and 0 < hi <= 0.5, name
        assert near_lo >= 1 and near_hi >= 1, name
        _, tol, exact = Sc.visc64(T, y, paras)
        assert bool(exact.any()) and bool((tol[~exact] > 0).all())


# ---- the mutants ------------------------------------------------------------------------------------------------------------
STEP_MUTANTS = ["no_heat", "heat_075", "central", "swap_upwind", "gr_by_dxl", "uniform_lap", "side_col0", "scale_u_only"]
GRID_MUTANTS = ["grid_row0", "stored_walls"]                       # only the stretched grid can catch these


@pytest.mark.parametrize("N,H,W,g", ALL_STEP)
def test_step_mutants_fail(N, H, W, g):
    c = Sc.step_case(N, H, W, g)
    s = c["vs"]
    dt = float(Sc.dt32(c, s))
    for raq in (c["raq"], c["raq_field"]):
        assert Sc.check_step(c, _good(c, dt, s, raq), dt, s, raq)[0] == []
        for m in STEP_MUTANTS:
            if m == "gr_by_dxl" and W == 3 and not g:
                continue                                       # one interior column between two walls: dxl == dxr on the uniform grid
            if m == "uniform_lap" and not g and (H, W) == (3, 3):
                continue                                       # ... where 0.5 dxr + 0.5 dxl is the uniform spacing itself
            assert Sc.check_step(c, _good(c, dt, s, raq, **{m: True}), dt, s, raq)[0], m
        for m in GRID_MUTANTS:
            if m == "grid_row0" and (H == 3 or W == 3):
                continue                                       # a single interior row or column
            fails = Sc.check_step(c, _good(c, dt, s, raq, **{m: True}), dt, s, raq)[0]
            assert bool(fails) == g, (m, "the uniform grid cannot tell" if g else "caught on the uniform grid?")
    if g and H > 3:
        assert Sc.dt32(c, s, row1_only=True) != Sc.dt32(c, s)          # dx_min from row 1 only
        assert Sc.check_dt(Sc.dt32(c, s, row1_only=True), c, s)[0]
    elif not g:
        assert Sc.dt32(c, s, row1_only=True) == Sc.dt32(c, s)          # (the uniform grid cannot tell)
    if N >= 2:
        assert Sc.check_dt(Sc.dt32(c, None), c, s)[0]                  # vel_scale ignored in the CFL step


def test_existing_adnet_gate_is_blind(golden):
    """test_hip_parity.test_adnet_step_vs_golden on its own inputs (128 x 506, uniform grid, RaQ 2.5, dt = 3e-7): a step without
    its heating term moves T_next by 7.5e-7 and passes the gate atol = 2e-6; the increment comparison rejects it."""
    H, W = 128, 506
    seed = int(golden("g14_adnet")["seeds"][0])
    xc, yc = Sc.grid_uniform(H, W)
    r = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    c = dict(N=1, H=H, W=W, xc=xc, yc=yc, u=r(fields.smooth_field(1, H, W, seed + 1) * 400.0),
             v=r(fields.smooth_field(1, H, W, seed + 2) * 400.0), T=fields.temperature_field(1, H, W, seed + 3), raq=np.array([2.5]))
    dt = float(np.float32(3e-7))
    good, mutant = _good(c, dt), _good(c, dt, no_heat=True)
    moved = float(np.abs(Sc.step64(c, dt, no_heat=True) - Sc.step64(c, dt)).max())
    print(f"\nthe heating term moves T_next by {moved:.3e}")
    assert 7.0e-7 <= moved <= 8.0e-7
    assert np.abs(mutant - Sc.step64(c, dt)).max() <= 2e-6                         # the existing gate passes it
    assert Sc.check_step(c, good, dt)[0] == [] and Sc.check_step(c, mutant, dt)[0]


@pytest.mark.parametrize("N,H,W", Sc.BUILD_SHAPES[1:])
def test_channel_mutants_fail(N, H, W):
    c = Sc.build_case(N, H, W)
    for unet in (False, True):
        ref = Sc.build_input_ref(c, unet)
        got = lambda ch: torch.stack([Sc.stored(r) for _, r, _ in ch], 1)  # noqa: E731
        assert Sc.check_channels(ref, got(ref))[0] == []
        for name, kw in (("yc where ycc belongs", dict(depth="yc")), ("the depth / 4", dict(quarter=True)), ("clip at 1e-7", dict(lo=1e-7))):
            assert Sc.check_channels(ref, got(Sc.build_input_ref(c, unet, **kw)))[0], name
    for C in (10, 12):
        x0 = Sc.roll_x0(c, C)
        for uv in (0, 1):
            ref, tol = Sc.roll_forward_ref(c, x0, uv)
            chk = lambda g: Lc.check_planes(["x"], [g], [ref], [tol])[0]  # noqa: E731
            assert chk(Sc.stored(ref)) == []
            assert chk(Sc.stored(Sc.roll_forward_ref(c, x0, 1 - uv)[0])), "update_v ignored"
        ref, tol = Sc.roll_forward_ref(c, x0, 1)
        for name, kw in (("ycc where yc belongs", dict(depth="ycc")), ("yc / 4", dict(quarter=True)), ("clip at 1e-7", dict(lo=1e-7))):
            assert Lc.check_planes(["x"], [Sc.stored(Sc.roll_forward_ref(c, x0, 1, **kw)[0])], [ref], [tol])[0], name


@pytest.mark.parametrize("H,W", Sc.ASM_SHAPES[1:])
def test_assembler_mutants_fail(H, W):
    S = Sc.store_case(H, W, 3)
    muts = (("ycc where yc belongs", dict(depth="ycc")), ("yc / 4", dict(quarter=True)), ("clip at 1e-7", dict(lo=1e-7)),
            ("targets scaled by s", dict(by_s=True)))
    seen = 0
    for i0, i1 in Sc.ASM_PAIRS[:2]:
        x, y = Sc.adtime_item_ref(S, i0, i1)[:2]
        assert Sc.check_item(x, Sc.as_got(x))[0] == [] and Sc.check_item(y, Sc.as_got(y))[0] == []
        clips = Sc.clip_shares(S["T"][i0:i0 + 1], S["yc"], S["paras"][i0:i0 + 1])[0] > 0
        for name, kw in muts:
            if "lo" in kw and not clips:
                continue                                       # (an item that never reaches 1e-8: the mutant does not apply)
            mx, my = Sc.adtime_item_ref(S, i0, i1, **kw)[:2]
            assert Sc.check_item(x, Sc.as_got(mx))[0] or Sc.check_item(y, Sc.as_got(my))[0], name
        assert Sc.check_item(y, Sc.as_got(Sc.adtime_item_ref(S, i0, i1, by_s=True)[1]))[0]
        x, y = Sc.newad_item_ref(S, i0)[:2]
        assert Sc.check_item(x, Sc.as_got(x))[0] == [] and Sc.check_item(y, Sc.as_got(y))[0] == []
        for name, kw in muts:
            if "lo" in kw and not clips:
                continue
            mx, my = Sc.newad_item_ref(S, i0, **kw)[:2]
            assert Sc.check_item(x, Sc.as_got(mx))[0] or Sc.check_item(y, Sc.as_got(my))[0], name
        seen += int(clips)
    assert seen >= 1
    s, tol = Sc.scaler64(S["paras"])
    assert bool((tol < 1e-5 * s).all()) and bool((tol > 0).all())
    s32 = np.float32(5.0) * np.exp(np.float32(1.80167667) * (S["paras"][:, 0].numpy().astype(np.float32) * np.float32(0.1))
                                   + np.log(S["paras"][:, 1].numpy().astype(np.float32)) * np.float32(0.4330392)
                                   + np.log(S["paras"][:, 2].numpy().astype(np.float32)) * np.float32(-0.46052953))
    assert bool(((Sc.t64(s32) - s).abs() <= tol).all())                            # an f32 evaluation lies within the bound

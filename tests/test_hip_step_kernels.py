"""The simulation-side kernels of csrc/loss.hip against f64, straight through the C ABI, at the shapes where they change path
(tests/step_cases.py: the case tables, the f64 references, the derived bounds, the comparison functions; tests/
test_step_cases_host.py puts the mutants of the references through the same comparisons on the CPU).

  1  the CFL step of mc_adnet_step: bit for bit the f32 evaluation of the header's expression, within 4 U of the f64 one
  2  mc_adnet_step: the increment T_next - T_prev per pixel within U (K_STEP M + E), exact walls, bit-equal side columns
  4  the viscosity channel of mc_ts_build_input, mc_ts_build_input_unet, mc_roll_forward_update and both assemblers
  5  the copied and scaled channels, bit for bit; the velocity scale against f64
  6  mc_roll_forward_update   7  mc_ts_wall_bc   8  mc_assemble_adtime_batch / mc_assemble_newad_batch
  9  the documented MC_EINVAL returns, which launch nothing

mc_rollout_dt and mc_rollout_step are bit-equal to mc_adnet_step on each member alone (tests/test_hip_rollout.py, on both grids
and at the size whose loops stride), so the f64 result of parts 1 and 2 carries over to them without a second comparison.

Every output lies between sentinel bands and is prefilled with NaN (an updated tensor: with a known field).  Every test prints its
worst err / bound (`pytest -s`); the figures measured on MI355X stand in DESIGN.md 4."""
import functools

import numpy as np
import pytest
import torch

import loss_cases as Lc
import step_cases as Sc
from pbml_mantle_convection_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5C
f32, i32 = torch.float32, torch.int32
NAN = float("nan")
MC_EINVAL = -1


class Guarded:
    """A tensor between two sentinel bands inside one larger allocation (restated from tests/test_hip_loss_kernels.py)."""

    def __init__(self, shape, dtype=f32, fill=NAN, guard_bytes=65536):
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.to(dtype))
        else:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.g

    def cpu(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[:self.g] == SENTINEL).all()), f"{what}: bytes BEFORE the buffer were overwritten"
        assert bool((self.raw[self.g + self.nbytes:] == SENTINEL).all()), f"{what}: bytes BEHIND the buffer were overwritten"
        return self.t.cpu()

    def still_nan(self, what):
        assert bool(torch.isnan(self.cpu(what)).all()), f"{what} was written"


def dev(a, dtype=f32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(DEV).contiguous()


def raw(name, *args):
    """The entry point's return code, not raised."""
    return getattr(L.load(), name)(*args)


def bits(t):
    return t.contiguous().view(torch.int32)


def report(tag, **worst):
    print(f"\n[{tag}] worst err / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---- 1, 2: the step ---------------------------------------------------------------------------------------------------------
def run_step(c, members, *, scaled, field, six, dt=None, ws=None, cn=Sc.CN):
    """mc_adnet_step on the members as one batch: (dt as np.float32, T_next [n, H, W] f64 numpy).  six: u, v are channels 0, 1 of a
    6-channel tensor whose other channels hold NaN (uv_stride = 6 H W), as ADNet.forward passes them."""
    n, H, W = len(members), c["H"], c["W"]
    if six:
        uv = torch.full((n, 6, H, W), NAN, dtype=f32)
        uv[:, 0], uv[:, 1] = torch.from_numpy(c["u"][members]).float(), torch.from_numpy(c["v"][members]).float()
        uv = uv.to(DEV)
        pu, pv, stride = uv.data_ptr(), uv.data_ptr() + 4 * H * W, 6 * H * W
    else:
        u, v = dev(c["u"][members]), dev(c["v"][members])
        pu, pv, stride = u.data_ptr(), v.data_ptr(), H * W
    T, xc, yc = dev(c["T"][members]), dev(c["xc"]), dev(c["yc"])
    vs = dev(c["vs"][members]) if scaled else None
    rq = dev(c["raq_field"][members]) if field else None
    rqs = None if field else dev(c["raq"][members])
    dt_io = Guarded((1,), fill=NAN if dt is None else float(dt))
    ws = Guarded((2,), i32, 0x12345678) if ws is None else ws
    out = Guarded((n, H, W))
    L.call("mc_adnet_step", pu, pv, stride, L.ptr(vs), L.ptr(T), L.ptr(rq), L.ptr(rqs), L.ptr(xc), L.ptr(yc), n, H, W, cn,
           int(dt is None), dt_io.ptr, ws.ptr, out.ptr, L.stream())
    got = out.cpu("T_next")
    ws.cpu("ws")
    return np.float32(dt_io.cpu("dt_io")[0].item()), got.double().numpy()


def _sub(c, members):
    """The case restricted to some members."""
    m = list(members)
    return dict(c, N=len(m), u=c["u"][m], v=c["v"][m], T=c["T"][m], raq_field=c["raq_field"][m], raq=c["raq"][m], vs=c["vs"][m])


STEP_PARAMS = [(N, H, W, g) for N, H, W in Sc.STEP_SHAPES for g in (False, True)]


@pytest.mark.parametrize("N,H,W,g", STEP_PARAMS)
def test_cfl_step(N, H, W, g):
    c = Sc.step_case(N, H, W, g)
    worst = 0.0
    groups = [list(range(N))] + ([[0]] if N > 1 else [])
    for members in groups:
        for scaled in (False, True):
            dt, _ = run_step(c, members, scaled=scaled, field=False, six=False)
            fails, w = Sc.check_dt(dt, _sub(c, members), c["vs"][members] if scaled else None)
            worst = max(worst, w)
            assert fails == [], (members, scaled, fails)
    if N > 1:
        # a batch wholly at rest: the diffusive limit, finite; and the scratch words of one call do not leak into the next
        # (cn = 1e-3 makes the moving member advection-limited at every shape, so that a leaked maximum would show)
        kw = dict(scaled=True, field=False, six=False, cn=1e-3)
        ws = Guarded((2,), i32, -1)
        rest, _ = run_step(c, [N - 1], ws=ws, **kw)
        dx = Sc.dt32(_sub(c, [N - 1]), None, cn=1e-3)
        assert np.isfinite(rest) and rest > 0 and rest.tobytes() == dx.tobytes()
        again, _ = run_step(c, [0], ws=ws, **kw)
        fresh, _ = run_step(c, [0], **kw)
        assert again.tobytes() == fresh.tobytes() and again < rest
        assert again.tobytes() == Sc.dt32(_sub(c, [0]), c["vs"][[0]], cn=1e-3).tobytes()
        back, _ = run_step(c, [N - 1], ws=ws, **kw)
        assert back.tobytes() == rest.tobytes()
    report(f"cfl {N}x{H}x{W} stretched={g}", dt=worst)


# (vel_scale given, RaQ as a field, six-channel stride, dt supplied as this share of the CFL step or None = computed)
STEP_COMBOS = [(True, False, False, None), (False, True, True, None), (True, True, True, 0.37), (False, False, False, 1.0)]


def _step_checks(c, combos):
    N = c["N"]
    members = list(range(N))
    worst = {}
    for scaled, field, six, share in combos:
        s = c["vs"] if scaled else None
        dt_in = None if share is None else np.float32(share * float(Sc.dt32(c, s)))
        dt, Tn = run_step(c, members, scaled=scaled, field=field, six=six, dt=dt_in)
        if dt_in is not None:
            assert dt.tobytes() == dt_in.tobytes()                     # a supplied dt is read, not written
        assert np.isfinite(Tn).all()
        fails, w = Sc.check_step(c, Tn, float(dt), s, c["raq_field"] if field else c["raq"])
        worst[f"s={int(scaled)} field={int(field)} six={int(six)} dt={'cfl' if share is None else share}"] = w
        assert fails == [], (scaled, field, six, share, fails)
    return worst


@pytest.mark.parametrize("N,H,W,g", STEP_PARAMS)
def test_step_increment_against_f64(N, H, W, g):
    report(f"step {N}x{H}x{W} stretched={g}", **_step_checks(Sc.step_case(N, H, W, g), STEP_COMBOS))


def test_step_whose_grid_strides():
    """513 x 520: 1042 blocks' worth of pixels on a grid capped at 1024.  Once, on the stretched grid, with everything switched on."""
    N, H, W = Sc.STEP_BIG
    c = Sc.step_case(N, H, W, True)
    dt, _ = run_step(c, [0], scaled=True, field=False, six=False)
    fails, w = Sc.check_dt(dt, c, c["vs"])
    assert fails == [], fails
    report(f"step {N}x{H}x{W} stretched", dt=w, **_step_checks(c, [(True, True, True, None)]))


# ---- 4, 5: the input builders -------------------------------------------------------------------------------------------------
def run_builder(c, unet):
    N, H, W = c["N"], c["H"], c["W"]
    t = {k: dev(c[k]) for k in ("T", "xc", "yc", "ycc", "paras", "nd", "dt", "up", "vp")}
    out = Guarded((N, 10 if unet else 7, H, W))
    if unet:
        L.call("mc_ts_build_input_unet", L.ptr(t["T"]), L.ptr(t["xc"]), L.ptr(t["yc"]), L.ptr(t["ycc"]), L.ptr(t["paras"]),
               L.ptr(t["nd"]), L.ptr(t["dt"]), L.ptr(t["up"]), L.ptr(t["vp"]), N, H, W, out.ptr, L.stream())
    else:
        L.call("mc_ts_build_input", L.ptr(t["T"]), L.ptr(t["xc"]), L.ptr(t["yc"]), L.ptr(t["ycc"]), L.ptr(t["paras"]), L.ptr(t["nd"]),
               N, H, W, out.ptr, L.stream())
    return out.cpu("out").double()


@pytest.mark.parametrize("unet", [False, True])
@pytest.mark.parametrize("N,H,W", Sc.BUILD_SHAPES + [Sc.BUILD_BIG])
def test_input_builders(N, H, W, unet):
    c = Sc.build_case(N, H, W)
    fails, worst = Sc.check_channels(Sc.build_input_ref(c, unet), run_builder(c, unet))
    report(f"{'mc_ts_build_input_unet' if unet else 'mc_ts_build_input'} {N}x{H}x{W}", V=worst)
    assert fails == [], fails


# ---- 6: the roll-forward update -----------------------------------------------------------------------------------------------
def _roll(c, C, update_v, four):
    N, H, W = c["N"], c["H"], c["W"]
    x0 = Sc.roll_x0(c, C)
    x = Guarded((N, C, H, W), fill=x0)
    if four:
        o = torch.full((N, 4, H, W), NAN, dtype=f32)
        o[:, 0], o[:, 1], o[:, 2] = c["u"].float(), c["v"].float(), c["Tn"].float()
        o = o.to(DEV)
        pu, pv, pT, stride = o.data_ptr(), o.data_ptr() + 4 * H * W, o.data_ptr() + 8 * H * W, 4 * H * W
    else:
        u, v, T = dev(c["u"]), dev(c["v"]), dev(c["Tn"])
        pu, pv, pT, stride = u.data_ptr(), v.data_ptr(), T.data_ptr(), H * W
    paras = dev(c["paras"])
    L.call("mc_roll_forward_update", x.ptr, C, pu, pv, pT, stride, L.ptr(paras), update_v, N, H, W, L.stream())
    ref, tol = Sc.roll_forward_ref(c, x0, update_v)
    return Lc.check_planes(["x"], [x.cpu("x").double()], [ref], [tol])


@pytest.mark.parametrize("N,H,W", Sc.BUILD_SHAPES)
def test_roll_forward_update(N, H, W):
    c = Sc.build_case(N, H, W)
    worst = {}
    for C, update_v, four in ((10, 1, False), (12, 0, True), (12, 1, True), (10, 0, False)):
        fails, w = _roll(c, C, update_v, four)
        worst[f"c={C} update_v={update_v} stride={'4HW' if four else 'HW'}"] = w
        assert fails == [], (C, update_v, four, fails)
    report(f"mc_roll_forward_update {N}x{H}x{W}", **worst)


def test_roll_forward_update_whose_grid_strides():
    fails, w = _roll(Sc.build_case(*Sc.BUILD_BIG), 12, 1, True)
    report("mc_roll_forward_update 1x513x520", V=w)
    assert fails == [], fails


# ---- 7: the wall condition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,W", Sc.WALL_SHAPES)
def test_wall_bc(N, H, W):
    src, ref = Sc.wall_case(N, H, W)
    out = Guarded((N, H, W))
    L.call("mc_ts_wall_bc", L.ptr(dev(src)), N, H, W, out.ptr, L.stream())
    got = out.cpu("t_out")
    assert not torch.isnan(got).any()                                  # the input's own walls are never read into the output
    assert torch.equal(bits(got), bits(ref.float()))


# ---- 8: the assemblers --------------------------------------------------------------------------------------------------------
def _store_dev(S, nan_from=None):
    uv = S["uv"].clone()
    if nan_from is not None:
        uv[:, nan_from:] = NAN                                         # planes the kernel must skip by the stride
    return {k: dev(v) for k, v in dict(T=S["T"], uv=uv, t=S["t"], paras=S["paras"], nd=S["nd"], xc=S["xc"], yc=S["yc"]).items()}


def run_adtime(S, D, pairs):
    b, H, W = len(pairs), S["H"], S["W"]
    o = dict(x=Guarded((b, 10, H, W)), y=Guarded((b, 3, H, W)), s=Guarded((b,)), p=Guarded((b, 3)))
    L.call("mc_assemble_adtime_batch", L.ptr(D["T"]), L.ptr(D["uv"]), L.ptr(D["t"]), L.ptr(D["paras"]), L.ptr(D["nd"]), L.ptr(D["xc"]),
           L.ptr(D["yc"]), L.ptr(dev(pairs, i32)), b, S["m"], S["cy"], H, W, o["x"].ptr, o["y"].ptr, o["s"].ptr, o["p"].ptr, L.stream())
    return {k: g.cpu(k) for k, g in o.items()}


def run_newad(S, D, idx):
    b, H, W = len(idx), S["H"], S["W"]
    o = dict(x=Guarded((b, 7, H, W)), y=Guarded((b, S["cy"], H, W)), tw=Guarded((b,)), s=Guarded((b,)))
    L.call("mc_assemble_newad_batch", L.ptr(D["T"]), L.ptr(D["uv"]), L.ptr(D["t"]), L.ptr(D["paras"]), L.ptr(D["nd"]), L.ptr(D["xc"]),
           L.ptr(D["yc"]), L.ptr(dev(idx, i32)), b, S["m"], S["cy"], H, W, o["x"].ptr, o["y"].ptr, o["tw"].ptr, o["s"].ptr, L.stream())
    return {k: g.cpu(k) for k, g in o.items()}


def _check_scale(s_got, s64, s_tol, worst):
    e = abs(float(s_got) - float(s64))
    worst["scaler"] = max(worst.get("scaler", 0.0), e / float(s_tol))
    assert e <= float(s_tol), (float(s_got), float(s64), float(s_tol))


@pytest.mark.parametrize("cy", [2, 3, 4])
@pytest.mark.parametrize("H,W", Sc.ASM_SHAPES)
def test_assemble_adtime(H, W, cy):
    S = Sc.store_case(H, W, cy)
    D = _store_dev(S, nan_from=2)
    got = run_adtime(S, D, Sc.ASM_PAIRS)
    worst = {}
    for b, (i0, i1) in enumerate(Sc.ASM_PAIRS):
        x, y, s64, s_tol, par = Sc.adtime_item_ref(S, i0, i1, s_kernel=got["s"][b])
        _check_scale(got["s"][b], s64, s_tol, worst)
        for n, ch, g in (("x", x, got["x"][b]), ("y", y, got["y"][b])):
            fails, w = Sc.check_item(ch, g.double())
            worst[n] = max(worst.get(n, 0.0), w)
            assert fails == [], (b, i0, i1, fails)
        assert torch.equal(bits(got["p"][b]), bits(par.float()))
    for b in (0, 3):                                                   # a slot depends on its item alone: a batch of one
        one = run_adtime(S, D, [Sc.ASM_PAIRS[b]])
        for k in ("x", "y", "s", "p"):
            assert torch.equal(bits(one[k][0]), bits(got[k][b])), (b, k)
    assert torch.equal(bits(got["x"][0]), bits(got["x"][2]))           # the repeated pair
    report(f"mc_assemble_adtime_batch {H}x{W} cy={cy}", **worst)


@pytest.mark.parametrize("cy", [2, 3])
@pytest.mark.parametrize("H,W", Sc.ASM_SHAPES)
def test_assemble_newad(H, W, cy):
    S = Sc.store_case(H, W, cy)
    D = _store_dev(S)
    got = run_newad(S, D, Sc.ASM_IDX)
    worst = {}
    for b, i0 in enumerate(Sc.ASM_IDX):
        x, y, s64, s_tol, tw = Sc.newad_item_ref(S, i0, s_kernel=got["s"][b])
        _check_scale(got["s"][b], s64, s_tol, worst)
        for n, ch, g in (("x", x, got["x"][b]), ("y", y, got["y"][b])):
            fails, w = Sc.check_item(ch, g.double())
            worst[n] = max(worst.get(n, 0.0), w)
            assert fails == [], (b, i0, fails)
        assert float(got["tw"][b]) == float(tw)
    for b in (0, 3):
        one = run_newad(S, D, [Sc.ASM_IDX[b]])
        for k in ("x", "y", "tw", "s"):
            assert torch.equal(bits(one[k][0]), bits(got[k][b])), (b, k)
    assert torch.equal(bits(got["x"][0]), bits(got["x"][2]))
    report(f"mc_assemble_newad_batch {H}x{W} cy={cy}", **worst)


# ---- 9: return codes that launch nothing --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _valid():
    """Device arrays of one small case for the argument checks."""
    c, b = Sc.step_case(3, 5, 6, False), Sc.build_case(3, 5, 6)
    t = {k: dev(c[k]) for k in ("u", "v", "T", "xc", "yc", "vs", "raq", "raq_field")}
    t.update({"b_" + k: dev(b[k]) for k in ("T", "xc", "yc", "ycc", "paras", "nd", "dt", "up", "vp")})
    return t


def _each(args, changes):
    """The argument list with one entry replaced, once per change."""
    for pos, val in changes:
        a = list(args)
        a[pos] = val
        yield pos, val, a


def test_einval_launches_nothing():
    t, s = _valid(), L.stream()
    N, H, W = 3, 5, 6
    p = {k: L.ptr(v) for k, v in t.items()}
    out, dt_io, ws = Guarded((6, 12, H, W)), Guarded((1,)), Guarded((2,), i32, 7)
    out_y, out_s, out_p = Guarded((6, 3, H, W)), Guarded((6,)), Guarded((6, 3))
    outs = (out, dt_io, out_y, out_s, out_p)

    def expect(name, args, changes):
        for pos, val, a in _each(args, changes):
            assert raw(name, *a) == MC_EINVAL, (name, pos, val)
        for g in outs:
            g.still_nan(name)
        assert bool((ws.cpu("ws") == 7).all()), name

    ad = [p["u"], p["v"], H * W, p["vs"], p["T"], None, p["raq"], p["xc"], p["yc"], N, H, W, Sc.CN, 1, dt_io.ptr, ws.ptr, out.ptr, s]
    expect("mc_adnet_step", ad, [(k, None) for k in (0, 1, 4, 7, 8, 14, 16)] + [(9, 0), (10, 2), (11, 2), (6, None), (15, None)])
    bi = [p["b_T"], p["b_xc"], p["b_yc"], p["b_ycc"], p["b_paras"], p["b_nd"], N, H, W, out.ptr, s]
    expect("mc_ts_build_input", bi, [(k, None) for k in (0, 1, 2, 3, 4, 5, 9)] + [(6, 0), (7, 0), (8, 0)])
    bu = bi[:6] + [p["b_dt"], p["b_up"], p["b_vp"], N, H, W, out.ptr, s]
    expect("mc_ts_build_input_unet", bu, [(k, None) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 12)] + [(9, 0), (10, 0), (11, 0)])
    rf = [out.ptr, 10, p["u"], p["v"], p["T"], H * W, p["b_paras"], 1, N, H, W, s]
    expect("mc_roll_forward_update", rf, [(k, None) for k in (0, 2, 3, 4, 6)] + [(1, 9), (5, H * W - 1), (8, 0), (9, 0), (10, 0)])
    wb = [p["T"], N, H, W, out.ptr, s]
    expect("mc_ts_wall_bc", wb, [(0, None), (4, None), (1, 0), (2, 1), (3, 2), (0, out.ptr)])
    S = Sc.store_case(5, 6, 3)
    D = _store_dev(S)
    pairs, idx = dev(Sc.ASM_PAIRS, i32), dev(Sc.ASM_IDX, i32)
    st = [L.ptr(D[k]) for k in ("T", "uv", "t", "paras", "nd", "xc", "yc")]
    aa = st + [L.ptr(pairs), 5, S["m"], 3, 5, 6, out.ptr, out_y.ptr, out_s.ptr, out_p.ptr, s]
    expect("mc_assemble_adtime_batch", aa, [(k, None) for k in list(range(8)) + [13, 14, 15, 16]] + [(8, 0), (9, 0), (10, 1), (11, 0), (12, 0)])
    an = st + [L.ptr(idx), 6, S["m"], 3, 5, 6, out.ptr, out_y.ptr, out_s.ptr, out_p.ptr, s]
    expect("mc_assemble_newad_batch", an, [(k, None) for k in list(range(8)) + [13, 14, 15, 16]] + [(8, 0), (9, 0), (10, 1), (10, 4), (11, 0), (12, 0)])

"""GPU, kernel level through the C ABI: the ensemble rollout's per-member CFL step, its advection-diffusion step, the stopping
rule and the six diagnostics (mc_rollout_*), against mc_adnet_step on each member alone at batch 1 (bit equality) and against
a numpy f64 evaluation of the same f32 fields.  Outputs are NaN-prefilled and sit between sentinel bands.  mc_adnet_step itself
is held against f64 in tests/test_hip_step_kernels.py; the bit equalities here carry that result over to mc_rollout_step."""
import functools

import numpy as np
import pytest
import torch

import eval_seams as S
import step_cases as Sc
from eval_seams import grid  # noqa: F401  (the uniform grid; test_hip_series_score imports it from here)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xA5


class Stretched(int):
    """A width whose case lives on the stretched, sheared grid of tests/step_cases.py (NaN in the stored wall coordinates)."""


# smallest interior; a row longer than a wave, ragged; several blocks a member; 130 x 260: the grid-stride loops run and the 128
# partials of a member take k_rollout_finalize through its second lane pass
SIZES = [(3, 5, 6), (2, 9, 70), (4, 33, 130), (2, 130, 260)]
CASES = SIZES + [pytest.param(4, 33, Stretched(130), id="4-33-130-stretched")]      # and the stretched grid at an existing size
# more members than k_rollout_finalize has waves, and more than one block of the per-member kernels (tests/eval_seams.py)
MEMBER_CASES = CASES + S.MEMBER_SHAPES
CN = 0.1


class Guarded:
    """A tensor between two sentinel bands inside one larger allocation."""

    def __init__(self, shape, dtype, fill, guard_bytes=65536):
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        self.t.fill_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.g] == SENTINEL).all()) and bool((self.raw[self.g + self.nbytes:] == SENTINEL).all())


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def case(B, H, W):
    return _case(B, H, int(W), isinstance(W, Stretched))


@functools.lru_cache(maxsize=None)
def _case(B, H, W, stretched):
    """Members with different fields, different vel_scale and different RaQ; the LAST member is at rest (u = v = 0)."""
    u, v, T = S.rollout_fields(B, H, W)
    vs, raq = S.member_scalars(B)
    xc, yc = Sc.grid_stretched(H, W) if stretched else grid(H, W)
    walls = tuple(a.astype(np.float32) for a in Sc.with_walls(xc, yc))            # what the kernels substitute, for the checks
    return dict(B=B, H=H, W=W, stretched=stretched, grid=walls, u=dev(u), v=dev(v), T=dev(T), vs=dev(vs), raq=dev(raq), xc=dev(xc),
                yc=dev(yc))


def adnet(c, idx, dt=None):
    """mc_adnet_step on the members idx as ONE batch: (dt f32 scalar, T_next [len(idx),H,W]) on the host."""
    from pbml_mantle_convection_amd import _lib as L
    n, H, W = len(idx), c["H"], c["W"]
    sel = lambda k: c[k][idx].contiguous()  # noqa: E731
    u, v, T, vs, raq = sel("u"), sel("v"), sel("T"), sel("vs"), sel("raq")
    dt_io = torch.full((1,), float("nan") if dt is None else float(dt), dtype=torch.float32, device=DEV)
    ws = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = Guarded((n, H, W), torch.float32, float("nan"))
    L.call("mc_adnet_step", L.ptr(u), L.ptr(v), H * W, L.ptr(vs), L.ptr(T), None, L.ptr(raq), L.ptr(c["xc"]), L.ptr(c["yc"]), n, H,
           W, CN, int(dt is None), L.ptr(dt_io), L.ptr(ws), out.ptr, L.stream())
    torch.cuda.synchronize()
    assert out.intact()
    return dt_io.cpu()[0], out.t.cpu()


def reference(B, H, W):
    return _reference(B, H, int(W), isinstance(W, Stretched))


@functools.lru_cache(maxsize=None)
def _reference(B, H, W, stretched):
    """Per member alone at batch 1: its own dt and next T; and the batch-wide dt of the whole batch.  Computed once."""
    c = _case(B, H, W, stretched)
    alone = [adnet(c, [b]) for b in range(B)]
    return dict(dt=torch.stack([a[0] for a in alone]), Tn=torch.cat([a[1] for a in alone]), dt_batch=adnet(c, list(range(B)))[0])


def rollout(c, idx, t0=None, t_end=None, steps0=None, n_rows=1, reps=1):
    """dx_min once, then reps times { mc_rollout_dt, mc_rollout_step, mc_rollout_finalize } on the members idx of the case."""
    from pbml_mantle_convection_amd import _lib as L
    n, H, W = len(idx), c["H"], c["W"]
    sel = lambda k: c[k][idx].contiguous()  # noqa: E731
    u, v, T, vs, raq = sel("u"), sel("v"), sel("T"), sel("vs"), sel("raq")
    nblk = L.call("mc_rollout_blocks", H, W)
    f64, i32 = torch.float64, torch.int32
    g = dict(dxm=Guarded((1,), torch.float32, float("nan")), ws=Guarded((n,), i32, -1), dt=Guarded((n,), f64, float("nan")),
             flags=Guarded((n,), i32, -1), Tn=Guarded((n, H, W), torch.float32, float("nan")),
             part=Guarded((n * nblk * 8,), f64, float("nan")), hist=Guarded((n_rows, n, 8), f64, float("nan")),
             t=Guarded((n,), f64, 0.0), te=Guarded((n,), f64, float("inf")), steps=Guarded((n,), i32, 0),
             cursor=Guarded((1,), i32, -1))
    if t0 is not None:
        g["t"].t.copy_(torch.tensor(t0, dtype=f64))
    if t_end is not None:
        g["te"].t.copy_(torch.tensor(t_end, dtype=f64))
    if steps0 is not None:
        g["steps"].t.copy_(torch.tensor(steps0, dtype=i32))
    s = L.stream()
    L.call("mc_rollout_set_cursor", g["cursor"].ptr, 0, n_rows, s)
    L.call("mc_rollout_dx_min", L.ptr(c["xc"]), H, W, g["dxm"].ptr, s)
    for _ in range(reps):
        L.call("mc_rollout_dt", L.ptr(u), L.ptr(v), H * W, L.ptr(vs), g["dxm"].ptr, g["t"].ptr, g["te"].ptr, n, H, W, CN, g["ws"].ptr,
               g["dt"].ptr, g["flags"].ptr, s)
        L.call("mc_rollout_step", L.ptr(u), L.ptr(v), H * W, L.ptr(vs), L.ptr(T), L.ptr(raq), L.ptr(c["xc"]), L.ptr(c["yc"]),
               g["dt"].ptr, g["flags"].ptr, n, H, W, g["Tn"].ptr, g["part"].ptr, s)
        L.call("mc_rollout_finalize", g["part"].ptr, g["dt"].ptr, g["flags"].ptr, g["te"].ptr, g["t"].ptr, g["steps"].ptr,
               g["cursor"].ptr, g["hist"].ptr, n_rows, n, H, W, s)
    torch.cuda.synchronize()
    for k, b in g.items():
        assert b.intact(), f"{k}: a kernel wrote outside its buffer"
    return {k: b.t.cpu().clone() for k, b in g.items()}


def free_run(B, H, W):
    return _free_run(B, H, int(W), isinstance(W, Stretched))


@functools.lru_cache(maxsize=None)
def _free_run(B, H, W, stretched):
    """One step of every member from t = 0 with no stopping time.  Computed once, shared, never modified."""
    return rollout(_case(B, H, W, stretched), list(range(B)))


def bits(a):
    return a.contiguous().view(torch.int64 if a.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("B,H,W", MEMBER_CASES)
def test_cfl_step_is_per_member(B, H, W):
    ref, got = reference(B, H, W), free_run(B, H, W)
    dt = got["dt"]
    assert torch.isfinite(dt).all() and (dt > 0).all()
    assert torch.equal(bits(dt.float()), bits(ref["dt"])), (dt, ref["dt"])         # bit equality with the member alone
    assert torch.equal(dt.float().double(), dt)                                    # an f32 value held in an f64
    dx = float(got["dxm"][0])
    xs = case(B, H, W)["grid"][0]                                                  # the case's own grid, walls substituted
    assert dx == float((xs[1:-1, 1:-1] - xs[1:-1, :-2]).min())
    dx2 = np.float32(dx) * np.float32(dx)
    diffusive = np.float32(0.5) * (dx2 * dx2) / (dx2 + dx2)
    assert float(dt[B - 1]) == float(diffusive)                                    # the member at rest: not NaN, not inf
    assert (dt[:B - 1] < float(diffusive)).all()                                   # the others are advection-limited
    assert len(set(dt.tolist())) == B                                              # and all different
    assert float(ref["dt_batch"]) == float(dt.min())                               # the batch-wide step is the slowest member's
    assert got["flags"].tolist() == [1] * B
    assert got["hist"][0, :, 1].tolist() == dt.tolist() and got["hist"][0, :, 0].tolist() == dt.tolist()
    assert got["t"].tolist() == dt.tolist() and got["steps"].tolist() == [1] * B and got["cursor"].tolist() == [1]
    for m in S.named_members(B):                               # a wave's second member; the last thread of block 0, the first of block 1
        assert float(dt[m]) == float(ref["dt"][m]) and int(got["flags"][m]) == 1 and int(got["steps"][m]) == 1, m
        assert float(got["t"][m]) == float(dt[m]) and got["hist"][0, m, :2].tolist() == [float(dt[m])] * 2, m
        assert float(dt[m]) != float(dt[m - 4]) and float(dt[m]) != float(dt[m - 1]), m


@pytest.mark.parametrize("B,H,W", MEMBER_CASES)
def test_step_equals_adnet_on_each_member_alone(B, H, W):
    ref, got = reference(B, H, W), free_run(B, H, W)
    assert not torch.isnan(got["Tn"]).any()
    for b in range(B):
        assert torch.equal(bits(got["Tn"][b]), bits(ref["Tn"][b])), f"member {b}: {(got['Tn'][b] - ref['Tn'][b]).abs().max()}"
    assert (got["Tn"][:, 0] == 1).all() and (got["Tn"][:, -1] == 0).all()
    assert torch.equal(got["Tn"][:, :, 0], got["Tn"][:, :, 1]) and torch.equal(got["Tn"][:, :, -1], got["Tn"][:, :, -2])
    for m in S.named_members(B):
        assert torch.equal(bits(got["Tn"][m]), bits(ref["Tn"][m])) and not torch.equal(got["Tn"][m], got["Tn"][m - 4]), m


@pytest.mark.parametrize("B,H,W", MEMBER_CASES)
def test_stopping_rule(B, H, W):
    c, ref = case(B, H, W), reference(B, H, W)
    dts = ref["dt"].double()
    role = S.roles(B, last=S.LAND)                             # member 0 frozen, member 1 landing; in the larger batches also 4 / 5
    frozen, landing = [b for b in range(B) if role[b] == S.FROZEN], [b for b in range(B) if role[b] == S.LAND]
    assert frozen[0] == 0 and landing[0] == 1 and (B <= 5 or (4 in frozen and 5 in landing))
    assert B <= 256 or (255 in frozen and 256 in landing)
    t0 = [1.0] * B
    t_end = [float("inf")] * B
    for b in frozen:
        t_end[b] = 0.5                                         # past its stopping time
    for b in landing:
        t_end[b] = 1.0 + 0.3 * float(dts[b])                   # crosses it within this step, every member at a time of its own
    steps0 = [5 + b for b in range(B)]
    got = rollout(c, list(range(B)), t0=t0, t_end=t_end, steps0=steps0)
    assert got["flags"].tolist() == role
    for b in frozen:
        # frozen: T copied, clock and count untouched, dt = 0 in the history row
        assert torch.equal(bits(got["Tn"][b]), bits(c["T"][b].cpu())), b
        assert float(got["t"][b]) == 1.0 and int(got["steps"][b]) == 5 + b and int(got["flags"][b]) == 0, b
        assert float(got["hist"][0, b, 1]) == 0.0 and float(got["hist"][0, b, 0]) == 1.0, b
    for b in landing:
        # landing: the clock is SET to t_end, the row holds t_end - t_before, the field took that (f32) step
        assert float(got["t"][b]) == t_end[b] and int(got["flags"][b]) == 2 and int(got["steps"][b]) == 6 + b, b
        short = t_end[b] - 1.0
        assert float(got["hist"][0, b, 1]) == short and float(got["hist"][0, b, 0]) == t_end[b], b
        assert 0 < short < float(dts[b]), b
        _, Tn1 = adnet(c, [b], dt=np.float32(short))
        assert torch.equal(bits(got["Tn"][b]), bits(Tn1[0])), b
        assert not torch.equal(got["Tn"][b], ref["Tn"][b]), b
    # the others step as if alone
    for b in range(2, B):
        if role[b] != S.STEP:
            continue
        assert torch.equal(bits(got["Tn"][b]), bits(ref["Tn"][b])), b
        assert float(got["t"][b]) == 1.0 + float(dts[b]) and int(got["steps"][b]) == 6 + b, b
    if B > 5:                                                  # both sides of the second member of a wave, by name
        assert got["flags"][3:6].tolist() == [1, 0, 2] and got["steps"][3:6].tolist() == [9, 9, 11]
        assert got["t"][4:6].tolist() == [1.0, t_end[5]]
    if B > 256:                                                # both sides of the block boundary of the per-member kernels
        assert got["flags"][252:].tolist() == [1, 2, 1, 0, 2] and got["steps"][252:].tolist() == [258, 259, 260, 260, 262]
        assert got["t"][253:].tolist() == [t_end[253], 1.0 + float(dts[254]), 1.0, t_end[256]]
        assert float(got["hist"][0, 256, 1]) == t_end[256] - 1.0 and float(got["dt"][256]) == t_end[256] - 1.0
    # a member that has landed is inactive from then on
    for b in landing:
        again = rollout(c, [b], t0=[t_end[b]], t_end=[t_end[b]], steps0=[7])
        assert int(again["flags"][0]) == 0 and float(again["dt"][0]) == 0.0 and float(again["t"][0]) == t_end[b], b
        assert torch.equal(bits(again["Tn"][0]), bits(c["T"][b].cpu())), b


@pytest.mark.parametrize("B,H,W", MEMBER_CASES)
def test_diagnostics_against_numpy_f64(B, H, W):
    c, got = case(B, H, W), free_run(B, H, W)
    Tn = got["Tn"].double().numpy()
    u, v, s = c["u"].cpu().double().numpy(), c["v"].cpu().double().numpy(), c["vs"].cpu().double().numpy()
    yc = c["grid"][1].astype(np.float64)
    h = got["hist"][0].numpy()
    assert np.isfinite(h).all()
    worst = [S.diagnostics_check(h[b], Tn[b], u[b], v[b], s[b], yc, b) for b in range(B)]      # sums within 1e-6 sum|terms|; min, max exact
    print(f"worst |got - want| / gate over {B} members: {max(worst):.3e} (member {int(np.argmax(worst))})")
    for m in S.named_members(B):
        assert worst[m] <= 1.0 and h[m, 6] == Tn[m].min() and h[m, 7] == Tn[m].max() and h[m, 2] != h[m - 4, 2], m
    assert h[B - 1, 3] == 0.0                                                      # the member at rest
    assert (h[:B - 1, 3] > 0).all()


@pytest.mark.parametrize("B,H,W", MEMBER_CASES)
def test_diagnostics_do_not_depend_on_the_batch(B, H, W):
    c, got = case(B, H, W), free_run(B, H, W)
    twice = rollout(c, list(range(B)))
    assert torch.equal(bits(twice["hist"]), bits(got["hist"]))                     # across two runs
    for b in range(B):
        alone = rollout(c, [b])
        assert torch.equal(bits(alone["hist"][0, 0]), bits(got["hist"][0, b])), b  # alone (B = 1) and inside the batch
        assert torch.equal(bits(alone["Tn"][0]), bits(got["Tn"][b]))
    order = list(range(B))[::-1]                                                   # and on its place in the batch
    rev = rollout(c, order)
    assert torch.equal(bits(rev["hist"][0].flip(0)), bits(got["hist"][0]))


def test_history_rows_follow_the_device_cursor():
    B, H, W = SIZES[1]
    c, one = case(B, H, W), free_run(B, H, W)
    got = rollout(c, list(range(B)), n_rows=2, reps=3)       # the third replay finds the cursor at n_steps: its row is dropped
    assert got["cursor"].tolist() == [2] and got["steps"].tolist() == [3] * B
    assert torch.equal(bits(got["hist"][0]), bits(one["hist"][0]))
    dt = one["dt"]
    assert got["hist"][1, :, 1].tolist() == dt.tolist()
    assert got["hist"][1, :, 0].tolist() == (dt + dt).tolist()
    assert torch.equal(bits(got["hist"][1, :, 2:]), bits(one["hist"][0, :, 2:]))   # (the same T_prev was stepped again)
    assert got["t"].tolist() == (dt + dt + dt).tolist()

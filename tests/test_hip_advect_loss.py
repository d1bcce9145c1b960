"""GPU, kernel level through the C ABI: the advection loss (mc_advect_loss_dt, mc_advect_loss of csrc/advect_loss.hip) against
the f64 reference of tests/advect_loss_ref.py -- the per-item time step bit for bit (the f32 evaluation of the header's
expression, and mc_rollout_dx_min + mc_rollout_dt), the weighted sum and every kept element of the increment of the gradient
planes within the derived bounds, exact zeros, untouched boundaries, bit-equal repeats and the MC_EINVAL cases.  Outputs sit
between sentinel bands; the gradient planes are channels 0 and 1 of a three-channel tensor (batch stride 3 H W) whose third
channel must stay as it was."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import advect_loss_ref as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0xA5
CASES = [(N, H, W) for N in A.BATCHES for (H, W) in A.SHAPES]
MC_S_T_PLAIN, MC_EINVAL = 5, -1


class Guarded:
    """A tensor between two sentinel bands inside one larger allocation."""

    def __init__(self, shape, dtype, fill, guard_bytes=65536):
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill)
        else:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.g] == SENTINEL).all()) and bool((self.raw[self.g + self.nbytes:] == SENTINEL).all())


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def desc(N, H, W, p_pred, norm, t_grad=-2):
    from pbml_mantle_convection_amd import _lib as L
    return L.LossDesc(N, H, W, int(p_pred), 0, 0, 0, int(norm == "l2"), 0.0, 126.0, 1.0, t_grad)


@functools.lru_cache(maxsize=None)
def run(N, H, W, cn, norm="l1", p_pred=True, shared=False, rep=0):
    """Both launches on a case (rep: a repeat, past the cache): (dt [N] f32, sums [16] f64, gradient tensor [N,3,H,W] f32, its
    prefill) on the host."""
    from pbml_mantle_convection_amd import _lib as L
    c = A.case(N, H, W, shared)
    ct = 3 if p_pred else 2
    x, uvp, s = dev(c["x"]), dev(c["uvp"][:, :ct]), dev(c["s"])
    y = dev(np.stack([c["up"], c["vp"], c["pp"]], 1))
    d = A.direct(c, A.dt32(c, cn), norm, p_pred)
    pre = A.prefill(N, H, W, max(np.abs(d["iu"]).max(), np.abs(d["iv"]).max()))
    g0 = np.stack([pre, -pre, 3.0 * pre], 1)
    g = dict(dt=Guarded((N,), torch.float32, float("nan")), ws=Guarded((L.ADVECT_WS_PER_ITEM * N,), torch.int32, -1),
             sums=Guarded((L.LOSS_SLOTS,), torch.float64, 0.0), gy=Guarded((N, 3, H, W), torch.float32, dev(g0)))
    ld = desc(N, H, W, p_pred, norm)
    st = L.stream()
    L.call("mc_advect_loss_dt", L.ptr(uvp), ct, L.ptr(x), 7, L.ptr(s), N, H, W, float(cn), g["ws"].ptr, g["dt"].ptr, st)
    L.call("mc_advect_loss", C.byref(ld), y.data_ptr(), y.data_ptr() + 4 * H * W, 3 * H * W, L.ptr(uvp), L.ptr(x), 7, L.ptr(s),
           g["dt"].ptr, g["sums"].ptr, g["gy"].ptr, g["gy"].ptr + 4 * H * W, st)
    torch.cuda.synchronize()
    assert all(v.intact() for v in g.values())
    return g["dt"].t.cpu().numpy(), g["sums"].t.cpu().numpy(), g["gy"].t.cpu().numpy(), g0.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(N, H, W, cn, norm, p_pred):
    c = A.case(N, H, W)
    return A.direct(c, A.dt32(c, cn), norm, p_pred)


def rollout_dt(xc, u, v, s, cn, H, W):
    """mc_rollout_dx_min + mc_rollout_dt on the members u, v [b,H,W] of ONE grid xc [H,W]: dt [b] as f32."""
    from pbml_mantle_convection_amd import _lib as L
    b = u.shape[0]
    dxm = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.zeros(b, dtype=torch.int32, device=DEV)
    dt = torch.full((b,), float("nan"), dtype=torch.float64, device=DEV)
    fl = torch.zeros(b, dtype=torch.int32, device=DEV)
    t, te = torch.zeros(b, dtype=torch.float64, device=DEV), torch.full((b,), float("inf"), dtype=torch.float64, device=DEV)
    L.call("mc_rollout_dx_min", L.ptr(xc), H, W, L.ptr(dxm), L.stream())
    L.call("mc_rollout_dt", L.ptr(u), L.ptr(v), H * W, L.ptr(s), L.ptr(dxm), L.ptr(t), L.ptr(te), b, H, W, float(cn), L.ptr(ws),
           L.ptr(dt), L.ptr(fl), L.stream())
    torch.cuda.synchronize()
    return dt.cpu().numpy().astype(np.float32)


@pytest.mark.parametrize("cn", [A.CN_REF, A.CN_ADV])
@pytest.mark.parametrize("N,H,W", CASES)
def test_time_step_is_the_rollouts_bit_for_bit(N, H, W, cn):
    """On the shared grid: one mc_rollout_dx_min and one mc_rollout_dt for the whole batch.  On a grid per item: the same two
    launches per item.  Both times also the f32 evaluation of the header's expression."""
    for shared in (True, False):
        c = A.case(N, H, W, shared)
        got = run(N, H, W, cn, shared=shared)[0]
        assert got.tobytes() == A.dt32(c, cn).tobytes(), (got, A.dt32(c, cn))
        xc = dev(4.0 * c["x"][:, 0])                                                # (exact; NaN in the stored wall columns)
        u, v, s = dev(c["uvp"][:, 0]), dev(c["uvp"][:, 1]), dev(c["s"])
        if shared:
            want = rollout_dt(xc[0], u, v, s, cn, H, W)
        else:
            want = np.concatenate([rollout_dt(xc[b], u[b:b + 1], v[b:b + 1], s[b:b + 1], cn, H, W) for b in range(N)])
        assert got.tobytes() == want.tobytes(), (got, want)
    if N > 1 and cn == A.CN_ADV:
        assert len(set(got.tolist())) == N                                          # the items' steps differ


@pytest.mark.parametrize("norm,cn,p_pred", [("l1", A.CN_REF, True), ("l1", A.CN_ADV, False), ("l2", A.CN_REF, False),
                                            ("l2", A.CN_ADV, True)])
@pytest.mark.parametrize("N,H,W", CASES)
def test_sum_and_gradient_increment_against_f64(N, H, W, norm, cn, p_pred):
    c = A.case(N, H, W)
    dt, sums, gy, g0 = run(N, H, W, cn, norm, p_pred)
    assert dt.tobytes() == A.dt32(c, cn).tobytes()                                  # the reference sees the kernel's dt
    d = reference(N, H, W, cn, norm, p_pred)
    err = abs(sums[MC_S_T_PLAIN] - d["sum"])
    print(f"\n{N}x{H}x{W} {norm} cn={cn}: sum {sums[MC_S_T_PLAIN]:.9e} ref {d['sum']:.9e} err {err:.2e} tol {d['sum_tol']:.2e}")
    assert err <= d["sum_tol"]
    assert not np.delete(sums, MC_S_T_PLAIN).any()                                  # no other slot
    ku, kv, share = A.keep_masks(reference(N, H, W, cn, "l1", p_pred))              # (the kink rules are on e itself)
    assert share <= A.MAX_SHARE
    for ch, (ref, bound, keep) in enumerate(((d["iu"], d["bu"], ku), (d["iv"], d["bv"], kv))):
        a0 = g0[:, ch].astype(np.float64)
        inc = gy[:, ch].astype(np.float64) - a0
        tol = bound + A.U * (np.abs(a0) + np.abs(a0 + ref))
        worst = float((np.abs(inc - ref) / tol)[keep].max())
        print(f"  channel {ch}: largest |error| / bound over {int(keep.sum())} kept pixels {worst:.3f}, "
              f"largest increment {np.abs(ref).max():.3e} beside |g0| <= {np.abs(a0).max():.3e}")
        assert worst <= 1.0
        assert np.abs(ref[keep]).max() > 100 * A.U * np.abs(a0).max()              # the increment is visible beside the prefill


@pytest.mark.parametrize("N,H,W", CASES)
def test_zeros_boundaries_and_repeats(N, H, W):
    c = A.case(N, H, W)
    for norm in ("l1", "l2"):
        dt, sums, gy, g0 = run(N, H, W, A.CN_REF, norm, True)
        for (i, j) in c["zeros_u"]:
            assert gy[:, 0, i, j].tobytes() == g0[:, 0, i, j].tobytes()            # u_p == 0: exactly no increment
        for (i, j) in c["zeros_v"]:
            assert gy[:, 1, i, j].tobytes() == g0[:, 1, i, j].tobytes()
        ring = np.ones((H, W), bool)
        ring[1:-1, 1:-1] = False
        assert gy[:, :2][:, :, ring].tobytes() == g0[:, :2][:, :, ring].tobytes()   # boundary rows and columns
        assert gy[:, 2].tobytes() == g0[:, 2].tobytes()                             # the third channel of the tensor
        for ch, planted in ((0, c["zeros_u"]), (1, c["zeros_v"])):                  # and the rest of the interior has moved
            free = np.ones((H, W), bool)
            free[0], free[-1], free[:, 0], free[:, -1] = False, False, False, False
            for (i, j) in planted:
                free[i, j] = False
            assert (gy[:, ch][:, free] != g0[:, ch][:, free]).mean() > 0.9
        again = run(N, H, W, A.CN_REF, norm, True, rep=1)
        assert again[0].tobytes() == dt.tobytes() and again[1].tobytes() == sums.tobytes() and again[2].tobytes() == gy.tobytes()


def test_invalid_arguments_launch_nothing():
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    N, H, W = 1, 5, 5
    c = A.case(N, H, W)
    x, uvp, s = dev(c["x"]), dev(c["uvp"]), dev(c["s"])
    y = dev(np.stack([c["up"], c["vp"], c["pp"]], 1))
    nan = float("nan")
    dt, ws = torch.full((N,), nan, device=DEV), torch.full((L.ADVECT_WS_PER_ITEM * N,), -1, dtype=torch.int32, device=DEV)
    sums = torch.zeros(L.LOSS_SLOTS, dtype=torch.float64, device=DEV)
    gy = torch.full((N, 3, H, W), 0.5, device=DEV)
    st = L.stream()
    good = [L.ptr(uvp), 3, L.ptr(x), 7, L.ptr(s), N, H, W, 2e4, L.ptr(ws), L.ptr(dt), st]
    for i, bad in ((0, None), (2, None), (4, None), (9, None), (10, None), (3, 6), (6, 4), (7, 4), (5, 0)):
        a = list(good)
        a[i] = bad
        assert lib.mc_advect_loss_dt(*a) == MC_EINVAL, i
    dt_ok = torch.full((N,), 0.25, device=DEV)
    u, v = y.data_ptr(), y.data_ptr() + 4 * H * W
    good = [None, u, v, 3 * H * W, L.ptr(uvp), L.ptr(x), 7, L.ptr(s), L.ptr(dt_ok), L.ptr(sums), gy.data_ptr(),
            gy.data_ptr() + 4 * H * W, st]
    ok = desc(N, H, W, True, "l1")
    for i in (1, 2, 4, 5, 7, 8, 9, 10, 11):
        a = list(good)
        a[0], a[i] = C.byref(ok), None
        assert lib.mc_advect_loss(*a) == MC_EINVAL, i
    assert lib.mc_advect_loss(*good) == MC_EINVAL                                   # no descriptor
    for d, xch in ((desc(N, 4, W, True, "l1"), 7), (desc(N, H, 4, True, "l1"), 7), (ok, 6), (desc(0, H, W, True, "l1"), 7)):
        a = list(good)
        a[0], a[6] = C.byref(d), xch
        assert lib.mc_advect_loss(*a) == MC_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(dt).all() and bool((ws == -1).all()) and not sums.any() and bool((gy == 0.5).all())
    # the fused one-launch loss and the momentum entry points keep refusing a descriptor without a temperature output
    d2 = desc(N, H, W, True, "l1")
    z = y.data_ptr()
    assert lib.mc_loss_fused(C.byref(d2), z, z, z, z, 3 * H * W, 3 * H * W, None, 0, 0, None, 0, L.ptr(uvp), None, None, None, None,
                             L.ptr(sums), z, z, z, z, 3 * H * W, 3 * H * W, None, st) == -2
    assert lib.mc_momentum_residual(C.byref(d2), z, z, z, z, 3 * H * W, 3 * H * W, z, z, z, L.ptr(sums), z, z, z, st) == MC_EINVAL

"""GPU, kernel level through the C ABI: the depth profiles, their time weights and sums (mc_ensemble_profiles) and the saves at
fixed simulated times (mc_ensemble_snapshot), on the fields of test_hip_rollout.case against the numpy f64 reference of
ensemble_stats_ref.  Outputs are NaN-prefilled (sums: prefilled with known values) and sit between sentinel bands."""
import functools

import numpy as np
import pytest
import torch

import ensemble_stats_ref as E
import eval_seams as S
from test_hip_rollout import CN, SIZES, Guarded, bits, case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A0, W0, N0 = 7.5, 3.25, 11           # non-zero prefill of acc, wsum, nacc
F64, I32 = torch.float64, torch.int32
# tests/eval_seams.py: a second member of a finalize wave and a second block of the per-member kernels; the row widths and
# heights at which the scoring kernels change path (the profiles are the row means those kernels restate)
MEMBER_SIZES = SIZES + S.MEMBER_SHAPES
PROFILE_SIZES = MEMBER_SIZES + S.WIDTH_SHAPES + S.CHUNK_SHAPES


class Profiles:
    """dx_min and mc_rollout_dt once (dt, flags of the members idx at the clocks t0 / t_end), then mc_ensemble_profiles as
    often as call() is used, on the same acc / wsum / nacc."""

    def __init__(self, c, idx, t0=None, t_end=None, prefill=(0.0, 0.0, 0)):
        from pbml_mantle_convection_amd import _lib as L
        self.c, self.n, H, W = c, len(idx), c["H"], c["W"]
        n = self.n
        sel = lambda k: c[k][idx].contiguous()  # noqa: E731
        self.u, self.v, self.T, self.vs = sel("u"), sel("v"), sel("T"), sel("vs")
        self.g = dict(dxm=Guarded((1,), torch.float32, float("nan")), ws=Guarded((n,), I32, -1), dt=Guarded((n,), F64, float("nan")),
                      flags=Guarded((n,), I32, -1), t=Guarded((n,), F64, 0.0), te=Guarded((n,), F64, float("inf")),
                      tas=Guarded((n,), F64, 0.0), prof=Guarded((n, 4, H), F64, float("nan")), acc=Guarded((n, 4, H), F64, prefill[0]),
                      wsum=Guarded((n,), F64, prefill[1]), nacc=Guarded((n,), I32, prefill[2]))
        g = self.g
        if t0 is not None:
            g["t"].t.copy_(torch.tensor(t0, dtype=F64))
        if t_end is not None:
            g["te"].t.copy_(torch.tensor(t_end, dtype=F64))
        s = L.stream()
        L.call("mc_rollout_dx_min", L.ptr(c["xc"]), H, W, g["dxm"].ptr, s)
        L.call("mc_rollout_dt", L.ptr(self.u), L.ptr(self.v), H * W, L.ptr(self.vs), g["dxm"].ptr, g["t"].ptr, g["te"].ptr, n, H, W, CN,
               g["ws"].ptr, g["dt"].ptr, g["flags"].ptr, s)

    def call(self, tas=None, with_prof=True):
        from pbml_mantle_convection_amd import _lib as L
        g, c = self.g, self.c
        if tas is not None:
            g["tas"].t.copy_(torch.tensor(tas, dtype=F64))
        L.call("mc_ensemble_profiles", L.ptr(self.u), L.ptr(self.v), c["H"] * c["W"], L.ptr(self.vs), L.ptr(self.T), g["dt"].ptr,
               g["flags"].ptr, g["t"].ptr, g["tas"].ptr, self.n, c["H"], c["W"], g["prof"].ptr if with_prof else None, g["acc"].ptr,
               g["wsum"].ptr, g["nacc"].ptr, L.stream())
        torch.cuda.synchronize()
        for k, b in g.items():
            assert b.intact(), f"{k}: a kernel wrote outside its buffer"
        return {k: b.t.cpu().clone() for k, b in g.items()}


@functools.lru_cache(maxsize=None)
def free_profiles(B, H, W):
    """One call on every member from t = 0, averaging from 0, sums prefilled with 0.  Computed once, shared, never modified."""
    return Profiles(case(B, H, W), list(range(B))).call()


@functools.lru_cache(maxsize=None)
def reference(B, H, W):
    c = case(B, H, W)
    return E.profiles(c["u"].cpu().numpy(), c["v"].cpu().numpy(), c["vs"].cpu().numpy(), c["T"].cpu().numpy())


@pytest.mark.parametrize("B,H,W", PROFILE_SIZES)
def test_profiles_against_numpy_f64(B, H, W):
    got = free_profiles(B, H, W)["prof"].numpy()
    want, mag = reference(B, H, W)
    assert got.shape == (B, 4, H) and np.isfinite(got).all()
    gate = 1e-12 * mag / W
    worst = 0.0
    for b in range(B):
        for q in range(4):
            d = np.abs(got[b, q] - want[b, q])
            i = int(np.argmax(d - gate[b, q]))
            print(f"member {b} {('T', 'u2', 'v2', 'vT')[q]} row {i}: got {got[b, q, i]!r} want {want[b, q, i]!r} |diff| {d[i]:.3e} "
                  f"gate {gate[b, q, i]:.3e}")
            worst = max(worst, float((d / np.maximum(gate[b, q], 1e-300)).max()))
    print(f"worst |got - want| / gate: {worst:.3e}")
    assert (np.abs(got - want) <= gate).all(), worst
    for m in S.named_members(B):                               # a row of block b * H / 4 far from block 0, by name
        assert (np.abs(got[m] - want[m]) <= gate[m]).all() and not np.array_equal(got[m], got[m - 4]), m
    assert (got[B - 1, 1:3] == 0).all() and (got[B - 1, 3] == 0).all()             # the member at rest
    assert (got[:B - 1, 1:3] > 0).all()
    # cross-check: the mean over the rows of the T profile is the all-cell mean of T (the history's T_mean convention)
    T = case(B, H, W)["T"].cpu().double().numpy()
    for b in range(B):
        val, ref, g = got[b, 0].mean(), T[b].sum() / (H * W), 1e-12 * np.abs(T[b]).sum() / (H * W)
        print(f"member {b}: mean of the T profile {val!r} all-cell mean {ref!r} |diff| {abs(val - ref):.3e} gate {g:.3e}")
        assert abs(val - ref) <= g, (b, val, ref, g)


@pytest.mark.parametrize("B,H,W", SIZES)
def test_profiles_do_not_depend_on_the_batch(B, H, W):
    c, got = case(B, H, W), free_profiles(B, H, W)
    twice = Profiles(c, list(range(B))).call()
    assert torch.equal(bits(twice["prof"]), bits(got["prof"]))                      # across two runs
    assert torch.equal(bits(twice["acc"]), bits(got["acc"]))
    for b in range(B):
        alone = Profiles(c, [b]).call()                                            # alone (B = 1) and inside the batch
        assert torch.equal(bits(alone["prof"][0]), bits(got["prof"][b])), b
        assert torch.equal(bits(alone["acc"][0]), bits(got["acc"][b])), b
    rev = Profiles(c, list(range(B))[::-1]).call()                                 # and on its place in the batch
    assert torch.equal(bits(rev["prof"].flip(0)), bits(got["prof"]))
    assert torch.equal(bits(rev["wsum"].flip(0)), bits(got["wsum"]))


@pytest.mark.parametrize("B,H,W", MEMBER_SIZES)
def test_time_weights(B, H, W):
    c = case(B, H, W)
    t0 = [1.0 + 0.125 * b for b in range(B)]
    d = free_profiles(B, H, W)["dt"].numpy()                                       # (dt does not depend on the clock)
    # averaging starts below t0 (and exactly at t0 for member 0): the whole step
    p = Profiles(c, list(range(B)), t0=t0)
    got = p.call(tas=[t0[0]] + [0.5] * (B - 1))
    assert got["dt"].numpy().tolist() == d.tolist() and got["flags"].tolist() == [1] * B
    assert got["wsum"].numpy().tolist() == d.tolist() and got["nacc"].tolist() == [1] * B
    # inside the step: the part of the step after t_avg_start
    ta = [t0[b] + 0.25 * d[b] for b in range(B)]
    want = [(np.float64(t0[b]) + d[b]) - np.float64(ta[b]) for b in range(B)]
    assert all(0 < want[b] < d[b] for b in range(B))
    got = Profiles(c, list(range(B)), t0=t0).call(tas=ta)
    assert got["wsum"].numpy().tolist() == want and got["nacc"].tolist() == [1] * B
    pr = got["prof"].numpy()
    assert np.array_equal(got["acc"].numpy(), np.asarray(want)[:, None, None] * pr)
    for m in S.named_members(B):                               # every member its own clock, step and averaging start
        assert float(got["wsum"][m]) == want[m] and int(got["nacc"][m]) == 1 and want[m] != want[m - 4], m
        assert np.array_equal(got["acc"][m].numpy(), want[m] * pr[m]) and float(got["t"][m]) == 1.0 + 0.125 * m, m
    # at the end of the step and beyond it: nothing is accumulated, the profile is still written
    q = Profiles(c, list(range(B)), t0=t0, prefill=(A0, W0, N0))
    got = q.call(tas=[t0[0] + d[0]] + [max(5.0, t0[b] + 2.0) for b in range(1, B)])      # (5.0, or beyond a later clock)
    assert (got["acc"] == A0).all() and (got["wsum"] == W0).all() and (got["nacc"] == N0).all()
    assert torch.equal(bits(got["prof"]), bits(free_profiles(B, H, W)["prof"]))


@pytest.mark.parametrize("B,H,W", MEMBER_SIZES)
def test_frozen_and_landing_members(B, H, W):
    c = case(B, H, W)
    d = free_profiles(B, H, W)["dt"].numpy()
    role = S.roles(B, last=S.FROZEN)                           # member 0 frozen, member 1 landing; in the larger batches also 4 / 5,
    frozen = [b for b in range(B) if role[b] == S.FROZEN]      # ... 253 landing, 255 and the one member of block 1 frozen
    landing = [b for b in range(B) if role[b] == S.LAND]
    t0 = [1.0] * B
    t_end = [float("inf")] * B
    for b in frozen:
        t_end[b] = 0.5                                         # past its stopping time
    for b in landing:
        t_end[b] = 1.0 + 0.3 * float(d[b])                     # crosses it within this step
    p = Profiles(c, list(range(B)), t0=t0, t_end=t_end, prefill=(A0, W0, N0))
    got = p.call(tas=[0.0] * B)
    assert got["flags"].tolist() == role and role[:2] == [0, 2]
    assert torch.equal(bits(got["prof"]), bits(free_profiles(B, H, W)["prof"]))
    pr = got["prof"].numpy()
    for b in frozen:
        # frozen: weight 0, its sums are bit-unchanged; its profile is still that of its field
        assert (got["acc"][b] == A0).all() and float(got["wsum"][b]) == W0 and int(got["nacc"][b]) == N0, b
    for b in landing:
        # landing: the f64 remainder t_end - t
        short = np.float64(t_end[b]) - np.float64(1.0)
        assert 0 < short < d[b] and float(got["dt"][b]) == short, b
        assert float(got["wsum"][b]) == W0 + short and int(got["nacc"][b]) == N0 + 1, b
        assert np.array_equal(got["acc"][b].numpy(), A0 + short * pr[b]), b
    for b in range(2, B):
        if role[b] != S.STEP:
            continue
        assert float(got["wsum"][b]) == W0 + d[b] and int(got["nacc"][b]) == N0 + 1, b
        assert np.array_equal(got["acc"][b].numpy(), A0 + d[b] * pr[b]), b
    if B > 5:                                                  # by name: both sides of index 4
        assert got["flags"][3:6].tolist() == [1, 0, 2] and got["nacc"][3:6].tolist() == [N0 + 1, N0, N0 + 1]
        assert float(got["wsum"][4]) == W0 and float(got["wsum"][5]) == W0 + (np.float64(t_end[5]) - 1.0)
    if B > 256:                                                # ... and of index 256
        assert got["flags"][253:].tolist() == [2, 1, 0, 0] and got["nacc"][253:].tolist() == [N0 + 1, N0 + 1, N0, N0]
        assert float(got["wsum"][254]) == W0 + d[254] and float(got["wsum"][256]) == W0 and (got["acc"][256] == A0).all()


@pytest.mark.parametrize("B,H,W", SIZES)
def test_accumulation_over_two_calls(B, H, W):
    c = case(B, H, W)
    d = free_profiles(B, H, W)["dt"].numpy()
    t0 = [1.0] * B
    p = Profiles(c, list(range(B)), t0=t0, prefill=(A0, W0, N0))
    ta2 = [1.0 + 0.5 * d[b] for b in range(B)]
    p.call(tas=[0.0] * B)                                                          # w1 = d
    got = p.call(tas=ta2, with_prof=False)                                         # w2 = (t0 + d) - ta2; prof = NULL: accumulate only
    pr = got["prof"].numpy()                                                       # (left by the first call)
    assert np.isfinite(pr).all()
    w1 = d
    w2 = np.array([(np.float64(1.0) + d[b]) - np.float64(ta2[b]) for b in range(B)])
    want = (A0 + w1[:, None, None] * pr) + w2[:, None, None] * pr
    assert np.array_equal(got["acc"].numpy(), want)
    assert np.array_equal(got["wsum"].numpy(), (W0 + w1) + w2) and got["nacc"].tolist() == [N0 + 2] * B


@pytest.mark.parametrize("B,H,W", MEMBER_SIZES)
def test_snapshot_rule(B, H, W):
    from pbml_mantle_convection_amd import _lib as L
    c = case(B, H, W)
    n, cap, reps = max(4, B), 2, 3                             # four members at every size; every member of the larger batches
    idx = [k % B for k in range(n)]
    # member m follows pattern m % 4 on a clock of its own: step d[m], saving time every[m]
    d = [(1e-3, 2e-3, 1.5e-3, 1e-3)[m % 4] * (1.0 + 0.25 * (m // 4)) for m in range(n)]
    every = [(1.5, 0.5, 0.0, 0.5)[m % 4] * d[m] for m in range(n)]       # steps 1 and 3; every step; never; (frozen)
    flags = [(E.STEP, E.LAND, E.STEP, E.FROZEN)[m % 4] for m in range(n)]
    assert d[:4] == [1e-3, 2e-3, 1.5e-3, 1e-3] and len(set(zip(d, every, flags))) == n
    clocks = [[(k + 1) * d[m] for k in range(reps)] for m in range(n)]
    # the host arithmetic of these conditions, before anything runs on the device
    rule = [E.save_rule(clocks[m], [flags[m]] * reps, every[m], cap) for m in range(n)]
    assert [r[0] for r in rule] == [([0, 2], [0, 1], [], [])[m % 4] for m in range(n)]
    assert [r[1] for r in rule] == [([], [2], [], [])[m % 4] for m in range(n)]
    g = dict(t=Guarded((n,), F64, float("nan")), flags=Guarded((n,), I32, -1), every=Guarded((n,), F64, 0.0),
             nxt=Guarded((n,), F64, 0.0), count=Guarded((n,), I32, 0), missed=Guarded((n,), I32, 0), slot=Guarded((n,), I32, -7),
             snaps=Guarded((n, cap, H, W), torch.float32, float("nan")), snap_t=Guarded((n, cap), F64, float("nan")))
    g["flags"].t.copy_(torch.tensor(flags, dtype=I32))
    g["every"].t.copy_(torch.tensor(every, dtype=F64))
    Tn = [(c["T"][idx] + 0.125 * (k + 1)).contiguous() for k in range(reps)]       # a different field after every step
    slots = []
    for k in range(reps):
        g["t"].t.copy_(torch.tensor([clocks[m][k] for m in range(n)], dtype=F64))
        L.call("mc_ensemble_snapshot", L.ptr(Tn[k]), g["t"].ptr, g["flags"].ptr, g["every"].ptr, g["nxt"].ptr, g["count"].ptr,
               g["missed"].ptr, g["slot"].ptr, cap, n, H, W, g["snaps"].ptr, g["snap_t"].ptr, L.stream())
        torch.cuda.synchronize()
        slots.append(g["slot"].t.cpu().tolist())
    for k, b in g.items():
        assert b.intact(), f"{k}: a kernel wrote outside its buffer"
    got = {k: b.t.cpu().clone() for k, b in g.items()}
    assert [s_[:4] for s_ in slots] == [[0, 0, -1, -1], [-1, 1, -1, -1], [1, -1, -1, -1]]
    assert slots == [[(0, 0, -1, -1)[m % 4] for m in range(n)], [(-1, 1, -1, -1)[m % 4] for m in range(n)],
                     [(1, -1, -1, -1)[m % 4] for m in range(n)]]
    assert got["count"].tolist() == [(2, 2, 0, 0)[m % 4] for m in range(n)]
    assert got["missed"].tolist() == [(0, 1, 0, 0)[m % 4] for m in range(n)]
    assert got["nxt"].tolist() == [float(r[2]) for r in rule]
    for m in S.named_members(n):                               # by name: the second member of a wave; thread 255 of block 0, thread 0 of block 1
        assert [s_[m] for s_ in slots] == [[0, -1, 1], [0, 1, -1], [-1, -1, -1], [-1, -1, -1]][m % 4], m
        assert int(got["count"][m]) == (2, 2, 0, 0)[m % 4] and float(got["nxt"][m]) == float(rule[m][2]), m
        assert m % 4 > 1 or float(got["nxt"][m]) != float(got["nxt"][m - 4]), m                   # (a member that saves: its own clock)
    if n > 256:
        assert got["snap_t"][256].tolist() == [clocks[256][0], clocks[256][2]] and got["count"][255:].tolist() == [0, 2]
    for m in range(n):
        for sl in range(cap):
            if sl < len(rule[m][0]):
                k = rule[m][0][sl]
                assert torch.equal(bits(got["snaps"][m, sl]), bits(Tn[k][m].cpu())), (m, sl)    # T_new of its step, bit for bit
                assert float(got["snap_t"][m, sl]) == clocks[m][k]                              # the member's own clock
            else:
                assert torch.isnan(got["snaps"][m, sl]).all() and torch.isnan(got["snap_t"][m, sl])   # untouched slots
    assert not torch.equal(got["snaps"][0, 1], got["snaps"][1, 1])

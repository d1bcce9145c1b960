"""CPU-only checks of the ensemble rollout's statistics: mc_ensemble_profiles / mc_ensemble_snapshot are declared, bound,
built and validate their arguments without a device; constructor and reset validation, broadcasting, the state's key set
with the options off and on, the command line; and the numpy reference (ensemble_stats_ref) the GPU tests reuse."""
import os
import re

import numpy as np
import pytest
import torch

import ensemble_stats_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_EINVAL = -1
A = 0x10000          # an aligned address that is never dereferenced: validation fails before any launch
ENTRY_POINTS = ("mc_ensemble_profiles", "mc_ensemble_snapshot")


def test_entry_points_declared_bound_and_built():
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import build_ext
    src = open(os.path.join(ROOT, "include", "mantle_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert set(re.findall(r"\b(mc_ensemble_[a-z0-9_]+)\s*\(", src)) == set(ENTRY_POINTS)
    lib = L.load()
    for name in ENTRY_POINTS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
        assert name not in L.VALUE_RETURNING                   # both launch kernels and return a status
    assert len(L.SIGNATURES["mc_ensemble_profiles"][1]) == 17 and len(L.SIGNATURES["mc_ensemble_snapshot"][1]) == 15
    assert "ensemble_stats.hip" in build_ext.SOURCES
    assert os.path.exists(os.path.join(build_ext.CSRC, "ensemble_stats.hip"))


def _prof(u=A, v=A, uvs=72, vs=A, T=A, dt=A, flags=A, t=A, tas=A, b=2, h=8, w=9, prof=A, acc=A, wsum=A, nacc=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_ensemble_profiles(u, v, uvs, vs, T, dt, flags, t, tas, b, h, w, prof, acc, wsum, nacc, None)


def _snap(Tn=A, t=A, flags=A, every=A, nxt=A, count=A, missed=A, slot=A, capacity=2, b=2, h=8, w=9, snaps=2 * A, snap_t=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_ensemble_snapshot(Tn, t, flags, every, nxt, count, missed, slot, capacity, b, h, w, snaps, snap_t, None)


def test_entry_points_validate_arguments_without_gpu():
    sizes = (dict(b=0), dict(b=-1), dict(b=65536), dict(h=4), dict(w=4), dict(h=0), dict(w=-3))
    for kw in (dict(u=None), dict(v=None), dict(T=None), dict(dt=None), dict(flags=None), dict(t=None), dict(tas=None),
               dict(acc=None), dict(wsum=None), dict(nacc=None), dict(uvs=71), dict(uvs=0), dict(uvs=-72)) + sizes:
        assert _prof(**kw) == MC_EINVAL, kw
    for kw in (dict(Tn=None), dict(t=None), dict(flags=None), dict(every=None), dict(nxt=None), dict(count=None),
               dict(missed=None), dict(slot=None), dict(snaps=None), dict(snap_t=None), dict(capacity=0), dict(capacity=-3),
               dict(snaps=A)) + sizes:                                                   # (snaps=A: T_new == snaps)
        assert _snap(**kw) == MC_EINVAL, kw


def test_constructor_and_reset_validation():
    from pbml_mantle_convection_amd import rollout as R
    T0, xc, yc = R.synthetic_ensemble(3, 6, 7, seed=4)
    paras = np.array([[1.5, 1e6, 10.0], [2.5, 1e7, 30.0], [4.0, 1e8, 60.0]])
    args = (torch.from_numpy(T0), xc, yc, yc, paras[:, 0], paras[:, 1], paras[:, 2], R.normalise_params(paras))
    net = torch.nn.Identity()
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            R.EnsembleRollout(net, "cpu", save_capacity=bad)
    off = R.EnsembleRollout(net, "cpu")
    assert off.profiles is False and off.save_capacity == 0
    # every refusal comes before anything touches a device
    with pytest.raises(ValueError, match="profiles=True"):
        off.reset(*args, t_avg_start=0.0)
    with pytest.raises(ValueError, match="save_capacity"):
        off.reset(*args, save_every=1e-3)
    with pytest.raises(ValueError, match="profiles=True"):
        R.EnsembleRollout(net, "cpu", save_capacity=2).reset(*args, t_avg_start=1e-3)
    with pytest.raises(ValueError, match="save_capacity"):
        R.EnsembleRollout(net, "cpu", profiles=True).reset(*args, save_every=1e-3)
    on = R.EnsembleRollout(net, "cpu", profiles=True, save_capacity=2)
    for kw in (dict(t_avg_start=-1e-3), dict(t_avg_start=float("nan")), dict(save_every=-1.0), dict(save_every=float("nan")),
               dict(t_avg_start=[0.0, 1.0]), dict(save_every=[1.0, 2.0, 3.0, 4.0]), dict(save_every=[1e-3, -1e-3, 1e-3])):
        with pytest.raises(ValueError):
            on.reset(*args, **kw)


def test_member_values_are_broadcast():
    from pbml_mantle_convection_amd import rollout as R
    z = R.broadcast_member_value(None, 3, "t_avg_start")
    assert z.dtype == torch.float64 and z.tolist() == [0.0] * 3
    assert R.broadcast_member_value(2e-4, 3, "save_every").tolist() == [2e-4] * 3
    assert R.broadcast_member_value(torch.tensor([1e-4]), 2, "x").dtype == torch.float64
    assert R.broadcast_member_value([1e-4, 0.0, float("inf")], 3, "x").tolist() == [1e-4, 0.0, float("inf")]
    assert R.broadcast_member_value(np.float32(0.5), 2, "x").tolist() == [0.5, 0.5]
    for bad in ([1.0, 2.0], float("nan"), -0.5, [0.0, -1.0, 0.0]):
        with pytest.raises(ValueError):
            R.broadcast_member_value(bad, 3, "x")
    assert R.PROFILE_NAMES == ("T", "u2", "v2", "vT")


def test_state_keys_with_options_off_and_on():
    from pbml_mantle_convection_amd import rollout as R
    T0, _, _ = R.synthetic_ensemble(3, 6, 7, seed=4)
    st = dict(T=torch.from_numpy(T0), t=torch.tensor([0.0, 1e-3, 0.3], dtype=torch.float64),
              t_end=torch.tensor([float("inf"), 2e-3, 0.25], dtype=torch.float64), steps=torch.tensor([0, 7, 9], dtype=torch.int32))
    off = R.EnsembleRollout(torch.nn.Identity(), "cpu").load_state(st)
    assert set(off.state()) == {"T", "t", "t_end", "steps"}                # exactly the parent's keys
    with pytest.raises(ValueError):
        off.load_state(dict(st, stats=dict(acc=torch.zeros(3, 4, 6), weight=torch.zeros(3), count=torch.zeros(3),
                                           next_save=torch.zeros(3))))
    for kw in (dict(profiles=True), dict(save_capacity=2), dict(profiles=True, save_capacity=2)):
        on = R.EnsembleRollout(torch.nn.Identity(), "cpu", **kw).load_state(st)
        got = on.state()
        assert set(got) == {"T", "t", "t_end", "steps", "stats"} and set(got["stats"]) == {"acc", "weight", "count", "next_save"}
        assert got["stats"]["acc"].shape == (3, 4, 6) and got["stats"]["acc"].dtype == torch.float64
        assert got["stats"]["count"].dtype == torch.int32 and got["stats"]["next_save"].dtype == torch.float64
        stats = dict(acc=torch.arange(72, dtype=torch.float64).view(3, 4, 6) / 7, weight=torch.tensor([0.1, 0.2, 0.3], dtype=torch.float64),
                     count=torch.tensor([1, 2, 3], dtype=torch.int32), next_save=torch.tensor([0.5, 0.0, 1e-3], dtype=torch.float64))
        back = on.load_state(dict(st, stats=stats)).state()["stats"]
        for k, v in stats.items():
            assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
        back["acc"].zero_()                                                # copies
        assert torch.equal(on.state()["stats"]["acc"], stats["acc"])
        assert torch.equal(on.load_state(st).state()["stats"]["acc"], stats["acc"])      # a state without stats leaves them
        with pytest.raises(ValueError):
            on.load_state(dict(st, stats=dict(stats, weight=stats["weight"][:2])))


def test_cli_arguments():
    from pbml_mantle_convection_amd import rollout as R
    base = "--params p.csv --steps 3 --out o --synthetic 2 32 48"
    a = R.build_arg_parser().parse_args(base.split())
    assert (a.profiles, a.t_avg_start, a.save_every, a.save_capacity) == (0, None, None, 0)
    a = R.build_arg_parser().parse_args((base + " --profiles 1 --t_avg_start 2e-4 --save_every 1e-4 --save_capacity 5").split())
    assert (a.profiles, a.t_avg_start, a.save_every, a.save_capacity) == (1, 2e-4, 1e-4, 5)


def test_reference_time_weight():
    d, t0 = 0.25, 1.0
    assert E.time_weight(E.STEP, t0, d, 0.0) == d and E.time_weight(E.STEP, t0, d, t0) == d          # ta <= t0: the whole step
    assert E.time_weight(E.STEP, t0, d, 1.0625) == (t0 + d) - 1.0625 == 0.1875                       # inside the step
    assert E.time_weight(E.STEP, t0, d, 1.25) == 0.0 and E.time_weight(E.STEP, t0, d, 2.0) == 0.0    # at its end and beyond
    assert E.time_weight(E.LAND, t0, 0.125, 0.5) == 0.125                                            # a landing step's remainder
    assert E.time_weight(E.FROZEN, t0, 0.0, 0.0) == 0.0 and E.time_weight(E.FROZEN, t0, d, 0.0) == 0.0
    # the weights of consecutive steps add up to t_final - ta (the identity the network-level test leans on)
    ts = np.cumsum([0.0, 0.25, 0.125, 0.5])
    assert sum(E.time_weight(E.STEP, ts[k], ts[k + 1] - ts[k], 0.3125) for k in range(3)) == ts[3] - 0.3125


def test_reference_profiles():
    rng = np.random.RandomState(3)
    u, v, T = (rng.standard_normal((2, 5, 7)).astype(np.float32) for _ in range(3))
    s = np.array([0.5, 3.0], np.float32)
    prof, mag = E.profiles(u, v, s, T)
    assert prof.shape == (2, 4, 5) and prof.dtype == np.float64 and mag.shape == (2, 4, 5)
    su = np.float64(np.float32(s[1] * v[1, 2, 3]))                         # one f32 product, then f64
    assert abs(prof[1, 0, 2] - T[1, 2].astype(np.float64).sum() / 7) <= 1e-15 * mag[1, 0, 2]
    assert abs(prof[1, 3, 2] - (np.float32(s[1] * v[1, 2]).astype(np.float64) * T[1, 2]).sum() / 7) <= 1e-15 * mag[1, 3, 2]
    assert (prof[:, 1:3] >= 0).all() and np.allclose(mag[:, 1:3], prof[:, 1:3] * 7, rtol=1e-14)
    assert su * su <= mag[1, 2, 2]


def test_reference_save_rule():
    d = 1e-3
    clocks, step = [d, 2 * d, 3 * d], [E.STEP] * 3
    assert E.save_rule(clocks, step, 1.5 * d, 2)[:2] == ([0, 2], [])                     # steps 1 and 3 only
    assert E.save_rule(clocks, step, 0.5 * d, 2)[:2] == ([0, 1], [2])                    # every step; the third is missed
    assert E.save_rule(clocks, step, 0.0, 2) == ([], [], 0.0)                            # save_every = 0: never
    assert E.save_rule(clocks, [E.FROZEN] * 3, 0.5 * d, 2) == ([], [], 0.0)              # a frozen member never saves
    assert E.save_rule(clocks, step, d, 2)[0] == [0, 2]                                  # strict >: t == next_save does not save
    assert E.save_rule(clocks, step, 0.5 * d, 2)[2] == 3 * d + 0.5 * d
    assert E.save_rule(clocks, step, 1.5 * d, 2, next_save=2.5 * d)[:2] == ([2], [])     # next_save carries over

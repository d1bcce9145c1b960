"""CPU-only checks of rollout scoring: mc_score_rollout is declared, exported, bound and built and validates its arguments
without a device; known answers of the numpy reference (rollout_score_ref) the GPU tests lean on; load_rollout_truth on a
temporary tree in the reference's layout; reset / constructor validation; summarise_rollout; the command lines."""
import os
import re

import numpy as np
import pytest
import torch

import rollout_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_EINVAL = -1
A = 0x10000          # an aligned address that is never dereferenced: validation fails before any launch
ENTRY = "mc_score_rollout"


def test_entry_point_declared_exported_bound_and_built():
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import build_ext
    src = open(os.path.join(ROOT, "include", "mantle_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert ENTRY in set(re.findall(r"\b(mc_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    assert ENTRY in L.SIGNATURES and hasattr(lib, ENTRY) and ENTRY not in L.VALUE_RETURNING
    assert len(L.SIGNATURES[ENTRY][1]) == 19
    assert "rollout_score.hip" in build_ext.SOURCES and os.path.exists(os.path.join(build_ext.CSRC, "rollout_score.hip"))
    assert ENTRY in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _score(Tp=A, Tn=2 * A, t=A, dt=A, flags=A, te=A, truth=A, tt=A, n=A, capacity=2, b=2, h=8, w=9, nxt=A, scored=A, skipped=A,
           table=A, prof=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_score_rollout(Tp, Tn, t, dt, flags, te, truth, tt, n, capacity, b, h, w, nxt, scored, skipped, table, prof, None)


def test_entry_point_validates_arguments_without_gpu():
    null = [dict([(k, None)]) for k in ("Tp", "Tn", "t", "dt", "flags", "te", "truth", "tt", "n", "nxt", "scored", "skipped", "table",
                                        "prof")]
    sizes = [dict(b=0), dict(b=-1), dict(b=65536), dict(h=4), dict(w=4), dict(h=0), dict(w=-3), dict(capacity=0), dict(capacity=-2)]
    for kw in null + sizes + [dict(Tn=A)]:                     # (Tn=A: T_prev == T_next)
        assert _score(**kw) == MC_EINVAL, kw


# ---- the reference module ------------------------------------------------------------------------------------------
def fields(seed=5, H=7, W=70):
    rng = np.random.RandomState(seed)
    return tuple((0.5 + 0.3 * rng.standard_normal((H, W))).astype(np.float32) for _ in range(3))


def test_reference_known_answers():
    Tp, Tn, Tr = fields()
    same = R.score_row(Tp, Tn, Tn, 0.25, 1.0)
    row = dict(zip(R.NAMES, same["row"]))
    assert row["mae"] == 0.0 and row["max_err"] == 0.0 and row["prof_mae"] == 0.0 and abs(row["corr"] - 1.0) <= same["gate"][4]
    assert row["t"] == 0.25 and row["theta"] == 1.0 and row["T_mean_pred"] == row["T_mean_true"]
    assert np.array_equal(same["prof"][0], same["prof"][1])
    # b = 2 a + 1 (exact in f32 for these a: a has 12 significant bits)
    a12 = (np.round(Tp * 1024) / 1024).astype(np.float32)
    lin = R.score_row(a12, a12, (2 * a12 + 1).astype(np.float32), 0.0, 0.0)
    assert abs(lin["row"][4] - 1.0) <= lin["gate"][4] < 1e-12 and abs(lin["row"][7] - (2 * lin["row"][6] + 1)) < 1e-14
    assert abs(lin["row"][2] - abs(a12.astype(np.float64) + 1).mean()) < 1e-14
    # a constant truth has no variance: corr is NaN, everything else is finite
    const = R.score_row(Tp, Tn, np.full_like(Tp, 0.375), 0.1, 0.5)
    assert np.isnan(const["row"][4]) and np.isnan(const["gate"][4]) and np.isfinite(np.delete(const["row"], 4)).all()
    assert const["row"][7] == 0.375 and (const["prof"][1] == 0.375).all()
    # against numpy on the interpolated field
    mid = R.score_row(Tp, Tn, Tr, 0.1, 0.5)
    a = R.interpolate(Tp, Tn, 0.5)
    assert np.array_equal(a, Tp.astype(np.float64) + 0.5 * (Tn.astype(np.float64) - Tp.astype(np.float64)))
    want = np.corrcoef(a.ravel(), Tr.astype(np.float64).ravel())[0, 1]
    assert abs(mid["row"][4] - want) < 1e-13
    assert abs(mid["row"][2] - np.abs(a - Tr).mean()) < 1e-15 and mid["row"][3] == np.abs(a - Tr).max()
    assert abs(mid["row"][5] - np.abs(a.mean(1) - Tr.astype(np.float64).mean(1)).mean()) < 1e-15
    assert abs(mid["row"][6] - a.mean()) < 1e-15 and (mid["gate"][[2, 5, 6, 7]] > 0).all() and (mid["gate"] < 1e-12).all()
    assert R.depth(7, 70) == 2 + 6 + 7 + 8 and R.depth(128, 506) == 8 + 6 + 128 + 8


def test_reference_crossing_rule():
    times = [0.0, 0.5, 1.0, 1.25, 3.0]
    due, sk, k = R.crossing(R.STEP, 0.0, 1.0, times, 5, 5, 0)
    assert [d[0] for d in due] == [0, 1, 2] and [float(d[2]) for d in due] == [0.0, 0.5, 1.0] and (sk, k) == (0, 3)
    assert R.crossing(R.STEP, 1.0, 1.125, times, 5, 5, 3) == ([], 0, 3)                     # nothing due
    due, sk, k = R.crossing(R.STEP, 1.5, 2.0, times, 5, 5, 1)                               # late times are skipped, not scored
    assert due == [] and (sk, k) == (3, 4)
    assert R.crossing(R.FROZEN, 0.0, 9.0, times, 5, 5, 0) == ([], 0, 0)
    assert R.crossing(R.STEP, 0.0, 9.0, times, 5, 2, 0)[2] == 2                             # n_truth > capacity is clamped
    assert R.crossing(R.STEP, 0.0, 9.0, times, 1, 5, 0)[2] == 1 and R.crossing(R.STEP, 0.0, 9.0, times, 0, 5, 0)[2] == 0
    assert R.end_of_step(R.LAND, 1.0, 0.25, 1.2) == 1.2 and R.end_of_step(R.STEP, 1.0, 0.25, 9.0) == 1.25
    assert R.end_of_step(R.FROZEN, 1.0, 0.0, 0.5) == 1.0
    due, _, _ = R.crossing(R.STEP, 1.0, 1.0, [1.0], 1, 1, 0)                                # a step of length 0: theta = 0
    assert float(due[0][2]) == 0.0


# ---- load_rollout_truth ----------------------------------------------------------------------------------------------
H0, W0 = 6, 8


def write_sim(root, an, num, n, seed, grid_shift=0.0, t0=0.0):
    d = os.path.join(root, an, f"sim_{num}")
    os.makedirs(d)
    rng = np.random.RandomState(seed)
    xs = np.linspace(0.1, 3.9, W0) + grid_shift
    ys = np.linspace(0.05, 0.95, H0)
    torch.save(torch.from_numpy(np.broadcast_to(xs[None, :], (H0, W0)).copy()), os.path.join(d, "xc.pt"))
    torch.save(torch.from_numpy(np.broadcast_to(ys[:, None], (H0, W0)).copy()), os.path.join(d, "yc.pt"))
    T = rng.standard_normal((n, 1, H0, W0))
    torch.save(torch.from_numpy(T), os.path.join(d, "e1_Tprev_data.pt"))
    times = t0 + np.cumsum(rng.uniform(0.5, 1.5, n + 2)) * 1e-3          # times.pt is longer than the series, as in the files
    torch.save(torch.from_numpy(times), os.path.join(d, "times.pt"))
    return T[:, 0].astype(np.float32), times


@pytest.fixture()
def tree(tmp_path):
    root = str(tmp_path)
    sims = [(3, "cv", 1.5, 1e6, 10.0, 0.0, 0.0, 0), (7, "cv", 4.0, 1e8, 60.0, 0.0, 0.0, 0), (9, "train", 2.0, 1e7, 30.0, 0.0, 0.0, 0)]
    torch.save(sims, os.path.join(root, "sims.pt"))
    data = {3: write_sim(root, "cv", 3, 5, 1, t0=0.25), 7: write_sim(root, "cv", 7, 8, 2), 9: write_sim(root, "train", 9, 3, 3, grid_shift=0.01)}
    return root, data


def test_load_rollout_truth(tree):
    from pbml_mantle_convection_amd.evaluate import load_rollout_truth
    from pbml_mantle_convection_amd.rollout import normalise_params
    root, data = tree
    a = load_rollout_truth(root, "cv")
    assert set(a) == {"T0", "xc", "yc", "ycc", "raq", "fkt", "fkp", "nd", "truth", "sim_ids"} and a["sim_ids"] == [3, 7]
    assert a["T0"].shape == (2, 1, H0, W0) and a["T0"].dtype == np.float32
    tr = a["truth"]
    assert tr["T"].shape == (2, 7, H0, W0) and tr["t"].shape == (2, 7) and tr["n"].tolist() == [4, 7]
    for m, num in enumerate((3, 7)):
        T, times = data[num]
        n = T.shape[0] - 1
        assert np.array_equal(a["T0"][m, 0], T[0]) and np.array_equal(tr["T"][m, :n], T[1:])
        assert np.array_equal(tr["t"][m, :n], times[1:n + 1] - times[0])              # snapshot i carries times[i]
        assert (tr["t"][m, n:] == np.inf).all() and (tr["T"][m, n:] == 0).all()      # padding
        assert (np.diff(tr["t"][m, :n]) > 0).all() and tr["t"][m, 0] > 0
    assert a["xc"][0, 0] == 0 and a["xc"][0, -1] == 4 and a["yc"][0, 0] == 0 and a["yc"][-1, 0] == 1    # the mesh training saw
    assert np.array_equal(a["nd"], normalise_params(np.array([[1.5, 1e6, 10.0], [4.0, 1e8, 60.0]])))
    assert a["raq"].tolist() == [1.5, 4.0] and a["fkp"].tolist() == [10.0, 60.0]
    # start, every, count
    b = load_rollout_truth(root, "cv", start=1, every=2, count=2)
    assert b["truth"]["n"].tolist() == [1, 2] and b["truth"]["T"].shape[1] == 2
    T7, t7 = data[7]
    assert np.array_equal(b["T0"][1, 0], T7[1]) and np.array_equal(b["truth"]["T"][1], T7[[3, 5]])
    assert np.array_equal(b["truth"]["t"][1], t7[[3, 5]] - t7[1])
    T3, t3 = data[3]
    assert np.array_equal(b["truth"]["T"][0, 0], T3[3]) and b["truth"]["t"][0].tolist() == [t3[3] - t3[1], np.inf]
    one = load_rollout_truth(root, "cv", sims=[7], every=3)
    assert one["sim_ids"] == [7] and np.array_equal(one["truth"]["T"][0], T7[[3, 6]])
    assert load_rollout_truth(root, "train")["sim_ids"] == [9]
    for kw in (dict(start=5), dict(start=-1), dict(every=0), dict(count=0), dict(sims=[4])):
        with pytest.raises(ValueError):
            load_rollout_truth(root, "cv", **kw)
    with pytest.raises(ValueError):
        load_rollout_truth(root, "train", start=2)                                    # no snapshot after the start


def test_load_rollout_truth_refuses_mixed_meshes(tree):
    from pbml_mantle_convection_amd.evaluate import load_rollout_truth
    root, _ = tree
    sims = torch.load(os.path.join(root, "sims.pt"), weights_only=True)
    write_sim(root, "cv", 11, 2, 4, grid_shift=0.01)
    torch.save(list(sims) + [(11, "cv", 2.0, 1e7, 30.0, 0.0, 0.0, 0)], os.path.join(root, "sims.pt"))
    with pytest.raises(ValueError, match="one mesh"):
        load_rollout_truth(root, "cv")
    assert load_rollout_truth(root, "cv", sims=[3, 7])["sim_ids"] == [3, 7]


def test_synthetic_rollout_truth():
    from pbml_mantle_convection_amd.evaluate import synthetic_rollout_truth
    from pbml_mantle_convection_amd.rollout import check_truth
    a = synthetic_rollout_truth(3, 4, 16, 24, seed=2)
    b = synthetic_rollout_truth(3, 4, 16, 24, seed=2)
    tr = a["truth"]
    assert tr["T"].shape == (3, 4, 16, 24) and tr["t"].shape == (3, 4) and tr["n"].tolist() == [4, 4, 4]
    assert np.array_equal(tr["T"], b["truth"]["T"]) and np.array_equal(tr["t"], b["truth"]["t"])
    assert (np.diff(tr["t"], axis=1) > 0).all() and (tr["t"] > 0).all()
    dx, dy = 4.0 / 22, 1.0 / 14
    limit = 0.5 * dx * dx * dy * dy / (dx * dx + dy * dy)
    assert (tr["t"][:, 1] - tr["t"][:, 0] < 0.1 * limit).all()                         # two times inside one CFL step
    check_truth(tr, 3, 16, 24, 4)
    assert a["T0"].shape == (3, 1, 16, 24) and len(set(a["raq"].tolist())) == 3


# ---- EnsembleRollout: constructor, reset, state ---------------------------------------------------------------------
def reset_args(B=3, H=6, W=7):
    from pbml_mantle_convection_amd import rollout as Ro
    T0, xc, yc = Ro.synthetic_ensemble(B, H, W, seed=4)
    paras = np.array([[1.5, 1e6, 10.0], [2.5, 1e7, 30.0], [4.0, 1e8, 60.0]])[:B]
    return (torch.from_numpy(T0), xc, yc, yc, paras[:, 0], paras[:, 1], paras[:, 2], Ro.normalise_params(paras))


def test_constructor_and_reset_validation():
    from pbml_mantle_convection_amd import rollout as Ro
    net = torch.nn.Identity()
    assert Ro.SCORE_NAMES == R.NAMES == ("t", "theta", "mae", "max_err", "corr", "prof_mae", "T_mean_pred", "T_mean_true")
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            Ro.EnsembleRollout(net, "cpu", score_capacity=bad)
    args = reset_args()
    T = np.zeros((3, 2, 6, 7), np.float32)
    t = np.array([[0.0, 1e-3], [1e-3, 2e-3], [5e-4, 6e-4]])
    off = Ro.EnsembleRollout(net, "cpu")
    assert off.score_capacity == 0
    with pytest.raises(ValueError, match="score_capacity"):
        off.reset(*args, truth=dict(T=T, t=t))                 # every refusal comes before anything touches a device
    on = Ro.EnsembleRollout(net, "cpu", score_capacity=2)
    bad = [dict(T=T[:2], t=t[:2]), dict(T=T[:, :, :5], t=t), dict(T=T[:, 0], t=t[:, 0]), dict(T=T, t=t[:, :1]), dict(T=T),
           dict(T=np.zeros((3, 3, 6, 7), np.float32), t=np.zeros((3, 3))),                                    # S > capacity
           dict(T=T, t=np.array([[0.0, 1e-3], [1e-3, 1e-3], [5e-4, 6e-4]])),                                  # not strictly ascending
           dict(T=T, t=np.array([[0.0, 1e-3], [2e-3, 1e-3], [5e-4, 6e-4]])),
           dict(T=T, t=np.array([[-1e-9, 1e-3], [1e-3, 2e-3], [5e-4, 6e-4]])),                                # negative
           dict(T=T, t=np.array([[0.0, np.nan], [1e-3, 2e-3], [5e-4, 6e-4]])),                                # not finite
           dict(T=T, t=np.array([[0.0, np.inf], [1e-3, 2e-3], [5e-4, 6e-4]])),
           dict(T=T, t=t, n=[2, 2]), dict(T=T, t=t, n=[2, 3, 2]), dict(T=T, t=t, n=[2, -1, 2]), [T, t]]
    for tr in bad:
        with pytest.raises(ValueError):
            on.reset(*args, truth=tr)
    # beyond n[m] anything goes: the padding of load_rollout_truth
    Tc, tc, nc = Ro.check_truth(dict(T=T, t=np.array([[0.0, np.inf], [1e-3, 2e-3], [np.inf, np.inf]]), n=[1, 2, 0]), 3, 6, 7, 2)
    assert Tc.dtype == torch.float32 and tc.dtype == torch.float64 and nc.dtype == torch.int32 and nc.tolist() == [1, 2, 0]
    assert Ro.check_truth(dict(T=T[:, :1], t=t[:, :1]), 3, 6, 7, 2)[2].tolist() == [1, 1, 1]      # S < capacity, n = None


def test_state_carries_the_scores():
    from pbml_mantle_convection_amd import rollout as Ro
    T0 = reset_args()[0]
    st = dict(T=T0, t=torch.tensor([0.0, 1e-3, 0.3], dtype=torch.float64), t_end=torch.full((3,), float("inf"), dtype=torch.float64),
              steps=torch.tensor([0, 7, 9], dtype=torch.int32))
    off = Ro.EnsembleRollout(torch.nn.Identity(), "cpu").load_state(st)
    assert set(off.state()) == {"T", "t", "t_end", "steps"} and off._sc is None
    score = dict(next=torch.tensor([1, 2, 0], dtype=torch.int32), scored=torch.tensor([1, 1, 0], dtype=torch.int32),
                 skipped=torch.tensor([0, 1, 0], dtype=torch.int32), table=torch.arange(48, dtype=torch.float64).view(3, 2, 8) / 7,
                 prof=torch.arange(72, dtype=torch.float64).view(3, 2, 2, 6) / 3)
    with pytest.raises(ValueError, match="score_capacity"):
        off.load_state(dict(st, score=score))
    on = Ro.EnsembleRollout(torch.nn.Identity(), "cpu", score_capacity=2).load_state(st)
    got = on.state()
    assert set(got) == {"T", "t", "t_end", "steps", "score"} and set(got["score"]) == {"next", "scored", "skipped", "table", "prof"}
    assert got["score"]["table"].shape == (3, 2, 8) and bool(torch.isnan(got["score"]["table"]).all())
    assert got["score"]["prof"].shape == (3, 2, 2, 6) and got["score"]["next"].tolist() == [0, 0, 0]
    back = on.load_state(dict(st, score=score)).state()["score"]
    for k, v in score.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
    back["table"].zero_()                                                  # copies
    assert torch.equal(on.state()["score"]["table"], score["table"])
    with pytest.raises(ValueError):
        on.load_state(dict(st, score=dict(score, table=score["table"][:, :1])))
    assert torch.equal(on.state()["score"]["next"], score["next"])         # a refused state changes nothing


# ---- summary and command lines ---------------------------------------------------------------------------------------
def test_summarise_rollout():
    from pbml_mantle_convection_amd.evaluate import summarise_rollout
    nan = float("nan")
    table = np.full((3, 4, 8), nan)
    #               t     theta mae   max   corr  pmae  Tp    Tt
    table[0, 0] = (1e-3, 0.5, 0.01, 0.1, 0.99, 0.001, 0.50, 0.51)
    table[0, 1] = (2e-3, 0.2, 0.03, 0.2, 0.95, 0.003, 0.52, 0.49)
    table[0, 2] = (3e-3, 1.0, 0.05, 0.3, 0.85, 0.005, 0.50, 0.50)
    table[0, 3] = (4e-3, 0.0, 0.07, 0.4, 0.92, 0.007, 0.54, 0.50)
    table[1, 0] = (1e-3, 0.5, 0.02, 0.1, 0.97, 0.002, 0.50, 0.50)
    table[1, 1] = (2e-3, 0.5, 0.04, 0.1, nan, 0.004, 0.50, 0.25)            # a NaN corr is not "below the level"
    s = summarise_rollout(dict(table=torch.from_numpy(table)))
    assert [d["member"] for d in s] == [0, 1, 2] and [d["scored"] for d in s] == [4, 2, 0]
    assert abs(s[0]["mae"] - 0.04) < 1e-15 and s[0]["corr_last"] == 0.92 and s[0]["prof_mae_last"] == 0.007
    assert abs(s[0]["T_mean_mae"] - (0.01 + 0.03 + 0.0 + 0.04) / 4) < 1e-15 and s[0]["horizon"] == 3e-3 and s[0]["t_last"] == 4e-3
    assert s[1]["horizon"] == float("inf") and np.isnan(s[1]["corr_last"]) and abs(s[1]["T_mean_mae"] - 0.125) < 1e-15
    assert s[2]["horizon"] == float("inf") and np.isnan(s[2]["mae"]) and np.isnan(s[2]["corr_last"])
    assert summarise_rollout(dict(table=table), level=0.96)[0]["horizon"] == 2e-3
    assert summarise_rollout(dict(table=table), level=0.5)[0]["horizon"] == float("inf")
    assert [d["member"] for d in summarise_rollout(dict(table=table), sim_ids=[3, 7, 9])] == [3, 7, 9]


def test_cli_arguments():
    from pbml_mantle_convection_amd import evaluate as Ev
    from pbml_mantle_convection_amd import rollout as Ro
    a = Ev.build_arg_parser().parse_args("--out o --synthetic 4 16 24".split())
    assert (a.rollout_steps, a.start, a.truth_every, a.truth_count, a.t_end, a.level) == (0, 0, 1, None, None, 0.9)
    a = Ev.build_arg_parser().parse_args("--out o --data_dir d --rollout_steps 50 --start 3 --truth_every 5 --truth_count 8 --t_end 1e-2".split())
    assert (a.rollout_steps, a.start, a.truth_every, a.truth_count, a.t_end) == (50, 3, 5, 8, 1e-2)
    base = "--params p.csv --steps 3 --out o --synthetic 2 32 48"
    r = Ro.build_arg_parser().parse_args(base.split())
    assert (r.truth, r.score_capacity) == (None, 0)
    r = Ro.build_arg_parser().parse_args((base + " --truth t.npz --score_capacity 6").split())
    assert (r.truth, r.score_capacity) == ("t.npz", 6)


def test_write_rollout_scores(tmp_path):
    from pbml_mantle_convection_amd.evaluate import summarise_rollout, write_rollout_scores
    score = dict(table=torch.full((2, 3, 8), float("nan"), dtype=torch.float64), prof=torch.zeros((2, 3, 2, 5), dtype=torch.float64),
                 scored=torch.tensor([1, 0], dtype=torch.int32), skipped=torch.zeros(2, dtype=torch.int32),
                 next=torch.tensor([1, 0], dtype=torch.int32))
    score["table"][0, 0] = torch.tensor([1e-3, 0.5, 0.01, 0.1, 0.99, 0.001, 0.5, 0.51], dtype=torch.float64)
    summary = dict(members=summarise_rollout(score, sim_ids=[3, 7]))
    npz, js = write_rollout_scores(str(tmp_path / "o"), score, summary, sim_ids=[3, 7])
    z = np.load(npz)
    assert set(z.files) == {"names", "sim", "table", "prof", "scored", "skipped", "next"} and z["sim"].tolist() == [3, 7]
    assert z["names"].tolist() == list(R.NAMES) and z["table"].shape == (2, 3, 8) and z["scored"].tolist() == [1, 0]
    import json
    lines = open(js).read().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["members"][0]["scored"] == 1

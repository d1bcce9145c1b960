"""GPU, through EnsembleRollout with score_capacity > 0: the small NewFluidNet, grid and members of test_hip_rollout_net.
Scoring leaves every other result bit-identical; graph replay equals eager launches, scores included; a rollout scored
against its own earlier states (at the end of a step and inside one); continuation through state() / load_state(); a member
that stops before its last truth time; scoring off; the command lines."""
import copy
import functools

import numpy as np
import pytest
import torch

import fields
import rollout_score_ref as R
from test_hip_rollout import bits
from test_hip_rollout_net import B, DEV, H, W, Scaled, eager6, grid, inputs, net, same

pytestmark = pytest.mark.gpu

CAP = 5                               # one slot more than the truth holds
SCORE_KEYS = ("table", "prof", "scored", "skipped", "next")


def rollout(use_graph=True, t_end=None, score_capacity=CAP, truth=None):
    from pbml_mantle_convection_amd.rollout import EnsembleRollout
    ro = EnsembleRollout(Scaled(copy.deepcopy(net()[0]).to(DEV)), DEV, use_graph=use_graph, score_capacity=score_capacity)
    xc, yc = grid()
    T0, paras, nd = inputs()
    kw = {} if truth is None else dict(truth={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in truth.items()})
    ro.reset(T0.clone(), xc.clone(), yc.clone(), yc.clone(), paras[:, 0].copy(), paras[:, 1].copy(), paras[:, 2].copy(), nd.copy(),
             t_end=t_end, **kw)
    return ro


@functools.lru_cache(maxsize=None)
def states():
    """(T [7,B,H,W] f32: the initial fields and the states after each of the six free steps, clocks [7,B] f64)."""
    ref = eager6()
    T = np.stack([inputs()[0].float().numpy()[:, 0]] + [t[:, 0].numpy() for t in ref["T"]])
    c = np.concatenate([np.zeros((1, B)), ref["hist"][:, :, 0].numpy()])
    assert (np.diff(c, axis=0) > 0).all()
    return T, c


def midpoint(k):
    """The f64 midpoint of the states k and k + 1, rounded to f32, at the midpoint of their clocks."""
    T, c = states()
    return (0.5 * (T[k].astype(np.float64) + T[k + 1].astype(np.float64))).astype(np.float32), 0.5 * (c[k] + c[k + 1])


@functools.lru_cache(maxsize=None)
def standard_truth():
    """Four snapshots per member: the member's own state after its 2nd step at that clock; the midpoint of its 3rd and 4th
    state; two foreign fields at 1/4 and 3/4 of its 6th step (two times inside one step)."""
    T, c = states()
    mid, tm = midpoint(3)
    other = fields.temperature_field(2 * B, H, W, 4321).astype(np.float32).reshape(B, 2, H, W)
    Tt = np.stack([T[2], mid, other[:, 0], other[:, 1]], 1)
    tt = np.stack([c[2], tm, c[5] + 0.25 * (c[6] - c[5]), c[5] + 0.75 * (c[6] - c[5])], 1)
    assert (np.diff(tt, axis=1) > 0).all()
    return dict(T=Tt, t=tt, n=None)


def cpu(o):
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def scored6(use_graph):
    """run(6) with the standard truth.  Computed once per mode, shared, never modified."""
    out = rollout(use_graph=use_graph, truth=standard_truth()).run(6)
    res = cpu({k: out[k] for k in ("T", "hist", "t", "steps")})
    res["score"] = cpu(out["score"])
    return res


def same_scores(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])) for k in SCORE_KEYS)


@pytest.mark.parametrize("use_graph", [True, False])
def test_scoring_changes_nothing_else(use_graph):
    ref, got = eager6(), scored6(use_graph)
    assert same(got["T"], ref["T"][5]) and same(got["hist"], ref["hist"]) and same(got["t"], ref["t"]) and same(got["steps"], ref["steps"])


def test_graph_replay_equals_eager():
    g, e = scored6(True), scored6(False)
    assert same_scores(g["score"], e["score"])
    s = g["score"]
    assert s["names"] == R.NAMES and s["table"].shape == (B, CAP, 8) and s["prof"].shape == (B, CAP, 2, H)
    assert s["scored"].tolist() == [4] * B and s["skipped"].tolist() == [0] * B and s["next"].tolist() == [4] * B
    assert bool(torch.isfinite(s["table"][:, :4]).all()) and bool(torch.isnan(s["table"][:, 4]).all())
    assert torch.equal(s["table"][:, :4, 0], torch.from_numpy(standard_truth()["t"]))
    th = s["table"][:, :, 1]
    assert (th[:, 0] == 1).all() and ((th[:, 2] > 0.2) & (th[:, 2] < 0.3)).all() and ((th[:, 3] > 0.7) & (th[:, 3] < 0.8)).all()


def test_rows_against_the_reference():
    """Every scored row of the standard run against rollout_score_ref on the host's copies of the states."""
    T, c = states()
    s, tr = scored6(True)["score"], standard_truth()
    step_of = (2, 4, 6, 6)                                    # the step (1-based) in which row k falls due
    for m in range(B):
        for k in range(4):
            j = step_of[k]
            tau = np.float64(tr["t"][m, k])
            theta = (tau - c[j - 1, m]) / (c[j, m] - c[j - 1, m])
            want = R.score_row(T[j - 1, m], T[j, m], tr["T"][m, k], tau, theta)
            got = s["table"][m, k].numpy()
            for q, name in enumerate(R.NAMES):
                print(f"member {m} row {k} {name}: got {got[q]!r} want {want['row'][q]!r} |diff| {abs(got[q] - want['row'][q]):.3e} "
                      f"gate {want['gate'][q]:.3e}")
            assert R.within(got, want["row"], want["gate"]), (m, k)
            assert R.within(s["prof"][m, k].numpy(), want["prof"], want["gate_prof"]), (m, k)


def test_self_consistency_at_the_end_of_a_step():
    """Fed with its own states at exactly their clocks the rollout scores theta = 1, no error, correlation 1."""
    T, c = states()
    steps = (1, 3, 4, 6)
    truth = dict(T=np.stack([T[j] for j in steps], 1), t=np.stack([c[j] for j in steps], 1), n=None)
    s = cpu(rollout(truth=truth).run(6)["score"])
    assert s["scored"].tolist() == [4] * B and s["skipped"].tolist() == [0] * B
    tab = s["table"].numpy()
    assert np.array_equal(tab[:, :4, 0], truth["t"]) and (tab[:, :4, 1] == 1).all()
    assert (tab[:, :4, 2] == 0).all() and (tab[:, :4, 3] == 0).all() and (tab[:, :4, 5] == 0).all()
    assert np.array_equal(tab[:, :4, 6], tab[:, :4, 7])
    for m in range(B):
        for k, j in enumerate(steps):
            gate = R.score_row(T[j - 1, m], T[j, m], T[j, m], c[j, m], 1.0)["gate"][4]
            print(f"member {m} step {j}: corr {tab[m, k, 4]!r} |1 - corr| {abs(tab[m, k, 4] - 1):.3e} gate {gate:.3e}")
            assert abs(tab[m, k, 4] - 1.0) <= gate


def test_self_consistency_inside_a_step():
    """Truth = the midpoint of two consecutive states at the midpoint of their clocks: what is left is the f32 rounding of the
    truth, at most half an f32 ulp of the larger value."""
    T, _ = states()
    pairs = (0, 2, 4)
    mids = [midpoint(k) for k in pairs]
    truth = dict(T=np.stack([a for a, _ in mids], 1), t=np.stack([t for _, t in mids], 1), n=None)
    s = cpu(rollout(truth=truth).run(6)["score"])
    assert s["scored"].tolist() == [3] * B
    tab = s["table"].numpy()
    for m in range(B):
        for r, k in enumerate(pairs):
            bound = 2.0 ** -24 * max(np.abs(T[k, m]).max(), np.abs(T[k + 1, m]).max())
            print(f"member {m} step {k + 1}: theta {tab[m, r, 1]!r} max_err {tab[m, r, 3]:.3e} bound {bound:.3e} mae {tab[m, r, 2]:.3e}")
            assert abs(tab[m, r, 1] - 0.5) < 1e-9 and 0 <= tab[m, r, 2] <= tab[m, r, 3] <= bound
    assert (tab[:, :3, 4] > 0.999999).all()


def test_state_round_trip_continues_to_the_same_scores():
    ref = scored6(True)
    ro = rollout(truth=standard_truth())
    a = cpu(ro.run(2)["score"])
    assert a["scored"].tolist() == [1] * B and bool(torch.isnan(a["table"][:, 1:]).all())
    st = ro.state()
    assert set(st["score"]) == {"next", "scored", "skipped", "table", "prof"}
    st = {k: ({j: w.cpu() for j, w in v.items()} if k == "score" else v.cpu()) for k, v in st.items()}
    ro.run(3)                                               # wander off (and score on), then come back
    out = ro.load_state(st).run(4)
    assert same(out["T"].cpu(), ref["T"]) and same(out["t"].cpu(), ref["t"]) and same_scores(cpu(out["score"]), ref["score"])
    # two runs in a row: the scores are cumulative since reset(), not cleared per run
    ro2 = rollout(truth=standard_truth())
    ro2.run(3)
    assert same_scores(cpu(ro2.run(3)["score"]), ref["score"])
    # reset() starts them again, and without a truth nothing is ever scored
    xc, yc = grid()
    T0, paras, nd = inputs()
    ro2.reset(T0.clone(), xc.clone(), yc.clone(), yc.clone(), paras[:, 0].copy(), paras[:, 1].copy(), paras[:, 2].copy(), nd.copy())
    s = cpu(ro2.run(6)["score"])
    assert s["scored"].tolist() == [0] * B and s["next"].tolist() == [0] * B and bool(torch.isnan(s["table"]).all())


def test_member_that_stops_before_its_last_truth_time():
    _, c = states()
    t_stop = float(c[2, 0]) + 0.5 * float(c[3, 0] - c[2, 0])        # inside member 0's third step, before its second truth time
    out = rollout(truth=standard_truth(), t_end=[t_stop, float("inf"), float("inf")]).run(6)
    s, free = cpu(out["score"]), scored6(True)["score"]
    assert out["steps"].tolist() == [3, 6, 6] and float(out["t"][0]) == t_stop
    assert s["scored"].tolist() == [1, 4, 4] and s["next"].tolist() == [1, 4, 4] and s["skipped"].tolist() == [0] * B
    assert bool(torch.isnan(s["table"][0, 1:]).all()) and bool(torch.isnan(s["prof"][0, 1:]).all())
    assert torch.equal(bits(s["table"][0, 0]), bits(free["table"][0, 0]))
    assert torch.equal(bits(s["table"][1:]), bits(free["table"][1:]))          # the other members do not notice
    # a truth time ON the stopping time is scored by the landing step with theta = 1
    tr = standard_truth()
    tt = tr["t"].copy()
    tt[0, 1] = t_stop
    land = cpu(rollout(truth=dict(T=tr["T"], t=tt, n=None), t_end=[t_stop, float("inf"), float("inf")]).run(6)["score"])
    assert land["scored"].tolist() == [2, 4, 4] and float(land["table"][0, 1, 0]) == t_stop and float(land["table"][0, 1, 1]) == 1.0


def test_scoring_off_allocates_nothing():
    ro = rollout(score_capacity=0)
    out = ro.run(1)
    assert out["score"] is None and ro._sc is None and set(ro.state()) == {"T", "t", "t_end", "steps"}
    assert same(out["T"].cpu(), eager6()["T"][0])


def test_rollout_cli_writes_scores(tmp_path):
    from pbml_mantle_convection_amd import rollout as Ro
    params = tmp_path / "params.csv"
    params.write_text("raq,fkt,fkp\n1.5,1e6,10\n4.0,1e8,60\n")
    T = fields.temperature_field(4, 32, 48, 77).astype(np.float32).reshape(2, 2, 32, 48)
    np.savez(tmp_path / "truth.npz", T=T, t=np.array([[0.0, 1e-12], [1e-12, 1.0]]), n=np.array([2, 2]))
    out = tmp_path / "out"
    base = f"--params {params} --steps 3 --synthetic 2 32 48 -l 2 -f 8 -r 2 -k 5 -p zeros"
    summary = Ro.main(f"{base} --out {out} --truth {tmp_path / 'truth.npz'} --score_capacity 3".split())
    z = np.load(out / "scores.npz")
    assert set(z.files) == {"names", "table", "prof", "scored", "skipped", "next"} and z["names"].tolist() == list(R.NAMES)
    assert z["table"].shape == (2, 3, 8) and z["prof"].shape == (2, 3, 2, 32) and z["scored"].tolist() == [2, 1] and z["next"].tolist() == [2, 1]
    assert z["table"][0, 0, 1] == 0 and np.isfinite(z["table"][0, :2]).all() and np.isnan(z["table"][1, 1:]).all()
    assert [d["scored"] for d in summary["score"]] == [2, 1] and summary["score"][0]["mae"] > 0
    out2 = tmp_path / "out2"
    plain = Ro.main(f"{base} --out {out2}".split())
    assert "score" not in plain and not (out2 / "scores.npz").exists()
    assert np.array_equal(np.load(out2 / "hist.npy"), np.load(out / "hist.npy"))


def test_evaluate_cli_scores_a_rollout(tmp_path):
    from pbml_mantle_convection_amd import evaluate as Ev
    out = tmp_path / "o"
    summary = Ev.main(f"--synthetic 2 32 48 --rollout_steps 12 --truth_count 4 -l 2 -f 8 -r 2 -k 5 -p zeros --out {out}".split())
    z = np.load(out / "rollout_scores.npz")
    assert z["table"].shape == (2, 4, 8) and z["prof"].shape == (2, 4, 2, 32) and z["names"].tolist() == list(R.NAMES)
    scored = (~np.isnan(z["table"][:, :, 0])).sum(1)
    assert summary["scored"] == scored.tolist() == z["scored"].tolist() and [d["scored"] for d in summary["members"]] == scored.tolist()
    assert (out / "rollout_summary.json").exists() and len(summary["t"]) == 2

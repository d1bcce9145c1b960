"""GPU, kernel level through the C ABI: mc_score_rollout on the fields of test_hip_rollout.case against the numpy f64
reference of rollout_score_ref, whose gates come from the magnitudes of the summed terms alone.  dt and flags come from
mc_rollout_dt and T_next from mc_rollout_step; every output is NaN-prefilled (counters: prefilled with known values) and sits
between sentinel bands that are checked after every call."""
import functools

import numpy as np
import pytest
import torch

import eval_seams as S
import fields
import rollout_score_ref as R
from test_hip_rollout import CN, SIZES, Guarded, bits, case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, I32 = torch.float32, torch.float64, torch.int32
NAN, INF = float("nan"), float("inf")
K0, S0 = 5, 7                         # non-zero prefill of scored, skipped
# tests/eval_seams.py: widths at which the lanes of rs_walk_row split between its two loops or take the main loop twice, heights
# of exactly one chunk and of one chunk and a row; batches with more than one block and more than four members
ROW_SIZES = SIZES + S.WIDTH_SHAPES + S.CHUNK_SHAPES
MEMBER_SIZES = SIZES + S.MEMBER_SHAPES


@functools.lru_cache(maxsize=None)
def truth_fields(n, cap, H, W):
    """[n, cap, H, W] f32 fields that differ from the case's temperatures.  Computed once, never modified."""
    return fields.temperature_field(n * cap, H, W, 9000 + H).astype(np.float32).reshape(n, cap, H, W)


class Scorer:
    """dx_min, mc_rollout_dt and mc_rollout_step once on the members idx at the clocks t0 / t_end (dt, flags, T_next); then
    truth(...) fills the truth buffers and call() runs mc_score_rollout on them."""

    def __init__(self, c, idx, cap, t0=None, t_end=None, nxt=0, scored=K0, skipped=S0):
        from pbml_mantle_convection_amd import _lib as L
        self.c, self.n, self.cap, H, W = c, len(idx), cap, c["H"], c["W"]
        n = self.n
        sel = lambda k: c[k][idx].contiguous()  # noqa: E731
        u, v, self.T, vs, raq = sel("u"), sel("v"), sel("T"), sel("vs"), sel("raq")
        nblk = L.call("mc_rollout_blocks", H, W)
        self.g = dict(dxm=Guarded((1,), F32, NAN), ws=Guarded((n,), I32, -1), dt=Guarded((n,), F64, NAN), flags=Guarded((n,), I32, -1),
                      t=Guarded((n,), F64, 0.0), te=Guarded((n,), F64, INF), Tn=Guarded((n, H, W), F32, NAN),
                      part=Guarded((n * nblk * 8,), F64, NAN), truth=Guarded((n, cap, H, W), F32, NAN), tt=Guarded((n, cap), F64, INF),
                      nt=Guarded((n,), I32, 0), next=Guarded((n,), I32, nxt), scored=Guarded((n,), I32, scored),
                      skipped=Guarded((n,), I32, skipped), table=Guarded((n, cap, 8), F64, NAN), prof=Guarded((n, cap, 2, H), F64, NAN))
        g = self.g
        if t0 is not None:
            g["t"].t.copy_(torch.tensor(t0, dtype=F64))
        if t_end is not None:
            g["te"].t.copy_(torch.tensor(t_end, dtype=F64))
        s = L.stream()
        L.call("mc_rollout_dx_min", L.ptr(c["xc"]), H, W, g["dxm"].ptr, s)
        L.call("mc_rollout_dt", L.ptr(u), L.ptr(v), H * W, L.ptr(vs), g["dxm"].ptr, g["t"].ptr, g["te"].ptr, n, H, W, CN, g["ws"].ptr,
               g["dt"].ptr, g["flags"].ptr, s)
        L.call("mc_rollout_step", L.ptr(u), L.ptr(v), H * W, L.ptr(vs), L.ptr(self.T), L.ptr(raq), L.ptr(c["xc"]), L.ptr(c["yc"]),
               g["dt"].ptr, g["flags"].ptr, n, H, W, g["Tn"].ptr, g["part"].ptr, s)
        torch.cuda.synchronize()
        self.t0, self.te = g["t"].t.cpu().numpy().copy(), g["te"].t.cpu().numpy().copy()
        self.dt, self.flags = g["dt"].t.cpu().numpy().copy(), g["flags"].t.cpu().numpy().copy()
        self.t1 = np.array([R.end_of_step(int(self.flags[m]), self.t0[m], self.dt[m], self.te[m]) for m in range(n)])
        self.Tp, self.Tn = self.T.cpu().numpy(), g["Tn"].t.cpu().numpy().copy()

    def truth(self, T, t, n):
        g = self.g
        g["truth"].t.copy_(torch.from_numpy(np.ascontiguousarray(T, dtype=np.float32)))
        g["tt"].t.copy_(torch.tensor(np.asarray(t, dtype=np.float64)))
        g["nt"].t.copy_(torch.tensor(n, dtype=I32))
        return self

    def state(self):
        return {k: b.t.cpu().clone() for k, b in self.g.items()}

    def call(self):
        """(outputs after the call, what the reference makes of the buffers as they stood before it)."""
        from pbml_mantle_convection_amd import _lib as L
        g, c = self.g, self.c
        b = {k: v.numpy() for k, v in self.state().items()}
        L.call("mc_score_rollout", L.ptr(self.T), g["Tn"].ptr, g["t"].ptr, g["dt"].ptr, g["flags"].ptr, g["te"].ptr, g["truth"].ptr,
               g["tt"].ptr, g["nt"].ptr, self.cap, self.n, c["H"], c["W"], g["next"].ptr, g["scored"].ptr, g["skipped"].ptr,
               g["table"].ptr, g["prof"].ptr, L.stream())
        torch.cuda.synchronize()
        for k, buf in g.items():
            assert buf.intact(), f"{k}: a kernel wrote outside its buffer"
        got = self.state()
        for k in ("dt", "flags", "t", "te", "Tn", "truth", "tt", "nt"):                 # inputs are inputs
            assert torch.equal(bits(got[k]), bits(torch.from_numpy(b[k]))), k
        want = R.step(self.Tp, b["Tn"], b["t"], b["dt"], b["flags"], b["te"], b["truth"], b["tt"], b["nt"], self.cap, b["next"],
                      b["scored"], b["skipped"], b["table"], b["prof"])
        return got, want


def check(got, want, rows=None):
    """Counters exactly, every table column and both profiles within the reference's gates; unwritten rows stay NaN."""
    for k in ("next", "scored", "skipped"):
        assert got[k].tolist() == want[k].tolist(), (k, got[k].tolist(), want[k].tolist())
    if rows is not None:
        assert sorted(want["rows"]) == sorted(rows), want["rows"]
    table, prof = got["table"].numpy(), got["prof"].numpy()
    for (m, k) in want["rows"]:
        for q, name in enumerate(R.NAMES):
            g_, w_, gate = table[m, k, q], want["table"][m, k, q], want["gate"][m, k, q]
            print(f"member {m} row {k} {name}: got {g_!r} want {w_!r} |diff| {abs(g_ - w_):.3e} gate {gate:.3e}")
        d = np.abs(prof[m, k] - want["prof"][m, k])
        i = np.unravel_index(int(np.argmax(d - want["gate_prof"][m, k])), d.shape)
        print(f"member {m} row {k} profiles: worst |diff| {d[i]:.3e} gate {want['gate_prof'][m, k][i]:.3e}")
    print(f"worst |got - want| / gate: table {S.worst_ratio(table, want['table'], want['gate']):.3e} "
          f"profiles {S.worst_ratio(prof, want['prof'], want['gate_prof']):.3e}")
    assert R.within(table, want["table"], np.nan_to_num(want["gate"], nan=0.0))
    assert R.within(prof, want["prof"], np.nan_to_num(want["gate_prof"], nan=0.0))
    written = np.zeros(table.shape[:2], bool)
    for (m, k) in want["rows"]:
        written[m, k] = True
        assert table[m, k, 0] == want["table"][m, k, 0] and table[m, k, 1] == want["table"][m, k, 1]      # t and theta: the same f64 ops
    assert np.isnan(table[~written]).all() and np.isnan(prof[~written]).all()


def clocks(n):
    return [1.0 + 0.125 * m for m in range(n)]


@pytest.mark.parametrize("B,H,W", ROW_SIZES)
def test_one_time_inside_the_step(B, H, W):
    s = Scorer(case(B, H, W), list(range(B)), 2, t0=clocks(B))
    assert s.flags.tolist() == [1] * B and (s.dt > 0).all()
    tt = np.stack([s.t0 + 0.3 * s.dt, s.t0 + 1.5 * s.dt], 1)
    got, want = s.truth(truth_fields(B, 2, H, W), tt, [2] * B).call()
    check(got, want, rows=[(m, 0) for m in range(B)])
    assert got["next"].tolist() == [1] * B and got["scored"].tolist() == [K0 + 1] * B and got["skipped"].tolist() == [S0] * B
    th = got["table"][:, 0, 1].numpy()
    assert ((th > 0.29) & (th < 0.31)).all()
    row = got["table"][:, 0].numpy()
    assert np.isfinite(row).all() and (row[:, 2] > 0).all() and (row[:, 3] >= row[:, 2]).all() and (np.abs(row[:, 4]) <= 1).all()


@pytest.mark.parametrize("B,H,W", ROW_SIZES)
def test_three_times_inside_one_step(B, H, W):
    s = Scorer(case(B, H, W), list(range(B)), 4, t0=clocks(B))
    tt = np.stack([s.t0 + f * s.dt for f in (0.25, 0.5, 0.75, 1.25)], 1)
    got, want = s.truth(truth_fields(B, 4, H, W), tt, [4] * B).call()
    check(got, want, rows=[(m, k) for m in range(B) for k in range(3)])
    assert got["next"].tolist() == [3] * B and got["scored"].tolist() == [K0 + 3] * B
    assert not torch.equal(got["table"][:, 0, 2:], got["table"][:, 1, 2:])           # three different truths, three different rows
    # the same call again: nothing more is due, nothing changes
    again, want2 = s.call()
    assert want2["rows"] == [] and all(torch.equal(bits(again[k]), bits(got[k])) for k in ("next", "scored", "skipped", "table", "prof"))


@pytest.mark.parametrize("B,H,W", SIZES)
def test_no_time_due_writes_nothing(B, H, W):
    s = Scorer(case(B, H, W), list(range(B)), 2, t0=clocks(B), nxt=1)
    tt = np.stack([s.t0 + 0.5 * s.dt, s.t0 + 2.0 * s.dt], 1)                         # row 0 lies before `next`, row 1 is not reached
    got, want = s.truth(truth_fields(B, 2, H, W), tt, [2] * B).call()
    check(got, want, rows=[])
    assert got["next"].tolist() == [1] * B and got["scored"].tolist() == [K0] * B and got["skipped"].tolist() == [S0] * B
    assert bool(torch.isnan(got["table"]).all()) and bool(torch.isnan(got["prof"]).all())


@pytest.mark.parametrize("B,H,W", SIZES)
def test_theta_zero_and_identical_fields(B, H, W):
    c = case(B, H, W)
    s = Scorer(c, list(range(B)), 2)                                                 # clocks at 0
    T = truth_fields(B, 2, H, W).copy()
    T[:, 0] = s.Tp                                                                   # the snapshot at time 0 IS the state
    tt = np.stack([np.zeros(B), 0.5 * s.dt], 1)
    got, want = s.truth(T, tt, [2] * B).call()
    check(got, want, rows=[(m, k) for m in range(B) for k in range(2)])
    row = got["table"][:, 0].numpy()
    assert (row[:, 0] == 0).all() and (row[:, 1] == 0).all()                         # tau == t0 == 0: theta == 0 exactly
    assert (row[:, 2] == 0).all() and (row[:, 3] == 0).all() and (row[:, 5] == 0).all()          # mae, max_err, prof_mae exactly 0
    assert (row[:, 6] == row[:, 7]).all() and torch.equal(bits(got["prof"][:, 0, 0]), bits(got["prof"][:, 0, 1]))
    assert (got["table"][:, 1, 1] == 0.5).all() and (got["table"][:, 1, 2] > 0).all()


@pytest.mark.parametrize("B,H,W", ROW_SIZES)
def test_theta_one_at_the_end_of_a_step_and_on_landing(B, H, W):
    c = case(B, H, W)
    free = Scorer(c, list(range(B)), 1, t0=clocks(B))
    t_end = [INF] * B
    t_end[1] = clocks(B)[1] + 0.3 * float(free.dt[1])                                # member 1 lands inside this step
    s = Scorer(c, list(range(B)), 1, t0=clocks(B), t_end=t_end)
    assert s.flags.tolist() == [1, 2] + [1] * (B - 2) and s.t1[1] == np.float64(t_end[1]) and 0 < s.dt[1] < free.dt[1]
    T = s.Tn[:, None].copy()                                                         # the truth IS the state after the step
    got, want = s.truth(T, s.t1[:, None], [1] * B).call()
    check(got, want, rows=[(m, 0) for m in range(B)])
    row = got["table"][:, 0].numpy()
    assert (row[:, 0] == s.t1).all() and (row[:, 1] == 1).all()                      # tau == t1: theta == 1 exactly
    assert (row[:, 2] == 0).all() and (row[:, 3] == 0).all()                         # identical fields: mae, max_err exactly 0
    assert got["next"].tolist() == [1] * B
    # one ulp beyond t1 is not due
    late = Scorer(c, list(range(B)), 1, t0=clocks(B), t_end=t_end)
    got, want = late.truth(T, np.nextafter(s.t1, INF)[:, None], [1] * B).call()
    check(got, want, rows=[])


@pytest.mark.parametrize("B,H,W", MEMBER_SIZES)
def test_late_times_frozen_members_and_counts(B, H, W):
    c = case(B, H, W)
    cap = 3
    t0 = clocks(B)
    t_end = [INF] * B
    pat = [m % 4 for m in range(B)]                                                  # beyond four members the four patterns repeat:
    for m in range(0, B, 4):
        t_end[m] = 0.5                                                               # 0, 4, ..., 256 are past their stopping time: frozen
    if B > 4:
        free = Scorer(c, list(range(B)), cap, t0=t0)
        for m in range(7, B, 4):
            t_end[m] = t0[m] + 0.9 * float(free.dt[m])                               # 7, 11, ..., 255 land inside this step
    s = Scorer(c, list(range(B)), cap, t0=t0, t_end=t_end)
    assert s.flags.tolist() == [0 if pat[m] == 0 else (2 if (pat[m] == 3 and m > 3) else 1) for m in range(B)]
    assert s.flags.tolist()[:4] == [0, 1, 1, 1][:B]
    # pattern 0: due times, but frozen.  pattern 1: a time the clock had passed (skipped), then one inside the step.
    # patterns 2, 3: n_truth = 0 (nothing counts) / n_truth = 1 of three due times.
    d = np.where(s.dt > 0, s.dt, 1e-6)                                               # (the frozen member's dt is 0)
    tt = np.stack([s.t0 - 0.25, s.t0 + 0.5 * d, s.t0 + 0.75 * d], 1)
    n = [(3, 3, 0, 1)[q] for q in pat]
    late = np.array([q >= 2 for q in pat])
    tt[late, 0] = s.t0[late] + 0.25 * s.dt[late]
    got, want = s.truth(truth_fields(B, cap, H, W), tt, n).call()
    rows = [r for m in range(B) for r in ([(m, 1), (m, 2)] if pat[m] == 1 else ([(m, 0)] if pat[m] == 3 else []))]
    assert rows[:3] == ([(1, 1), (1, 2)] + ([(3, 0)] if B > 3 else []))[:3]
    check(got, want, rows=rows)
    assert got["next"].tolist() == [(0, 3, 0, 1)[q] for q in pat]
    assert got["scored"].tolist() == [(K0, K0 + 2, K0, K0 + 1)[q] for q in pat] and got["skipped"].tolist() == [(S0, S0 + 1, S0, S0)[q] for q in pat]
    assert bool(torch.isnan(got["table"][0]).all()) and bool(torch.isnan(got["table"][1, 0]).all())      # frozen; the late row
    if B > 5:                                                                        # by name: a workgroup beyond the first four
        assert bool(torch.isnan(got["table"][4]).all()) and int(got["scored"][4]) == K0 and int(got["next"][4]) == 0
        assert int(got["scored"][5]) == K0 + 2 and int(got["skipped"][5]) == S0 + 1 and bool(torch.isfinite(got["table"][5, 1:, :4]).all())
        assert bool(torch.isnan(got["table"][5, 0]).all()) and float(got["table"][5, 1, 0]) == tt[5, 1] != tt[1, 1]
    if B > 256:                                                                      # ... the landing 255 and the frozen 256, whose dt and
        assert int(s.flags[255]) == 2 and int(s.flags[256]) == 0                     # flags thread 0 of block 1 of k_rollout_dt wrote
        assert int(got["scored"][255]) == K0 + 1 and int(got["next"][255]) == 1 and float(got["table"][255, 0, 0]) == tt[255, 0]
        assert s.t1[255] == np.float64(t_end[255]) and 0 < s.dt[255] < free.dt[255]  # (the landing step is the shorter one, and
        assert abs(float(got["table"][255, 0, 1]) - 0.25) < 1e-6                     # theta is taken on its own length)
        assert bool(torch.isnan(got["table"][256]).all()) and int(got["scored"][256]) == K0 and int(got["skipped"][256]) == S0


@pytest.mark.parametrize("B,H,W", SIZES)
def test_n_truth_beyond_the_capacity_is_clamped(B, H, W):
    s = Scorer(case(B, H, W), list(range(B)), 2, t0=clocks(B))
    tt = np.stack([s.t0 + 0.25 * s.dt, s.t0 + 0.5 * s.dt], 1)
    got, want = s.truth(truth_fields(B, 2, H, W), tt, [5] * B).call()                # (the sentinel bands sit where row 2 would be)
    check(got, want, rows=[(m, k) for m in range(B) for k in range(2)])
    assert got["next"].tolist() == [2] * B and got["scored"].tolist() == [K0 + 2] * B


@pytest.mark.parametrize("B,H,W", SIZES)
def test_constant_truth_has_no_correlation(B, H, W):
    s = Scorer(case(B, H, W), list(range(B)), 1, t0=clocks(B))
    T = np.full((B, 1, H, W), 0.3, np.float32)
    got, want = s.truth(T, (s.t0 + 0.5 * s.dt)[:, None], [1] * B).call()
    check(got, want, rows=[(m, 0) for m in range(B)])
    row = got["table"][:, 0].numpy()
    assert np.isnan(row[:, 4]).all() and np.isfinite(np.delete(row, 4, axis=1)).all()
    assert (row[:, 7] == np.float64(np.float32(0.3))).all() and (got["prof"][:, 0, 1] == float(np.float32(0.3))).all()


@pytest.mark.parametrize("B,H,W", ROW_SIZES + S.MEMBER_SHAPES)
def test_rows_do_not_depend_on_the_batch(B, H, W):
    c = case(B, H, W)
    T = truth_fields(B, 2, H, W)

    def run(idx):
        s = Scorer(c, idx, 2, t0=[clocks(B)[m] for m in idx])
        tt = np.stack([s.t0 + 0.25 * s.dt, s.t0 + 0.6 * s.dt], 1)
        return s.truth(T[idx], tt, [2] * len(idx)).call()[0]

    whole = run(list(range(B)))
    assert bool(torch.isfinite(whole["table"][:, :, :4]).all())
    for m in range(B):
        alone = run([m])                                                             # alone (b = 1) and inside the batch
        assert torch.equal(bits(alone["table"][0]), bits(whole["table"][m])), m
        assert torch.equal(bits(alone["prof"][0]), bits(whole["prof"][m])), m
    for m in S.named_members(B):
        assert not torch.equal(whole["table"][m, :, 2:4], whole["table"][m - 4, :, 2:4]), m      # another member, another row
    rev = run(list(range(B))[::-1])                                                  # and on its place in the batch
    assert torch.equal(bits(rev["table"].flip(0)), bits(whole["table"])) and torch.equal(bits(rev["prof"].flip(0)), bits(whole["prof"]))

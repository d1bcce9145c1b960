"""The seams of the evaluation kernels (csrc/rollout.hip, ensemble_stats.hip, rollout_score.hip, series_score.hip): their launch
arithmetic restated as pure functions of (B or N, H, W), the shapes that take every path of it, and numpy f64 restatements of
the sums in the kernels' own order with the mutants that stay inside one path.  Device-free: nothing here imports torch or the
library.  The constants are read out of the .hip sources, so a changed constant changes the classes below and fails
tests/test_eval_seams_host.py on the CPU before it can take a shape off the path it is listed for."""
import math
import os
import re

import numpy as np

import fields
import rollout_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbml_mantle_convection_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _ints(name, pattern):
    found = re.findall(pattern, source(name))
    assert len(found) == 1, (name, pattern, found)                 # the expression exists once: it is the one that is launched
    return tuple(int(x) for x in (found[0] if isinstance(found[0], tuple) else (found[0],)))


def read_constants():
    """Every number the path classes depend on, from the expression in the source that uses it."""
    c = {}
    c["SS_CHUNK"], = _ints("series_score.hip", r"enum \{ SS_CHUNK = (\d+) \};")
    c["SS_LANES"], = _ints("series_score.hip", r"__launch_bounds__\((\d+)\) void k_series_finalize\(")
    c["GATHER_THREADS"], c["GATHER_CAP"] = _ints("series_score.hip", r"dim3 grid\(max\(1, min\(cdiv\(h \* w, (\d+)\), (\d+)\)\), b\);")
    c["GATHER_BLOCK"], = _ints("series_score.hip", r"hipLaunchKernelGGL\(k_series_build_input, grid, dim3\((\d+)\),")
    c["RS_WAVES"], c["RS_CHUNK"] = _ints("rollout_score.hip", r"enum \{ RS_WAVES = (\d+), RS_CHUNK = (\d+), RS_COLS = \d+ \};")
    c["WALK_AHEAD"], c["WALK_MAIN"] = _ints("rollout_score.hip", r"for \(; j \+ (\d+) < W; j \+= (\d+)\) \{")
    c["WALK_TAIL"], = _ints("rollout_score.hip", r"for \(; j < W; j \+= (\d+)\) \{")
    c["WALK_QUADS"], c["WALK_LANES"] = _ints("rollout_score.hip", r"for \(int q = 0; q < (\d+); \+\+q\) \{ pv\[q\] = p\[j \+ (\d+) \* q\];")
    c["FIN_THREADS"], = _ints("rollout.hip", r"hipLaunchKernelGGL\(k_rollout_finalize, dim3\(1\), dim3\((\d+)\),")
    fin = re.findall(r"for \(int b = threadIdx\.x >> 6; b < B; b \+= blockDim\.x >> 6\) \{", source("rollout.hip"))
    assert len(fin) == 1                                           # wave w takes members w, w + (threads / 64), ...
    c["FIN_LANE_STRIDE"], = _ints("rollout.hip", r"for \(int k = lane; k < nblk; k \+= (\d+)\) \{")
    c["RO_THREADS"], c["RO_CAP"] = _ints("rollout.hip", r"int ro_blocks\(int h, int w\) \{ return max\(1, min\(cdiv\(h \* w, (\d+)\), (\d+)\)\); \}")
    per_member = [("rollout.hip", "k_rollout_ws_init"), ("rollout.hip", "k_rollout_dt"), ("ensemble_stats.hip", "k_ensemble_save_rule")]
    sizes = {_ints(f, r"hipLaunchKernelGGL\(%s, dim3\(cdiv\(b, (\d+)\)\), dim3\((\d+)\)," % k) for f, k in per_member}
    assert len(sizes) == 1, sizes                                  # the three per-member kernels share one block size
    c["MEMBER_DIV"], c["MEMBER_BLOCK"] = sizes.pop()
    return c


C = read_constants()
EXPECTED = dict(SS_CHUNK=64, SS_LANES=64, GATHER_THREADS=256, GATHER_CAP=1024, GATHER_BLOCK=256, RS_WAVES=16, RS_CHUNK=128,
                WALK_AHEAD=192, WALK_MAIN=256, WALK_TAIL=64, WALK_QUADS=4, WALK_LANES=64, FIN_THREADS=256, FIN_LANE_STRIDE=64,
                RO_THREADS=256, RO_CAP=128, MEMBER_DIV=256, MEMBER_BLOCK=256)      # what the shape tables below were chosen for
FIN_WAVES = C["FIN_THREADS"] // 64


def cdiv(a, b):
    return -(-a // b)


# ---- the launch arithmetic, path class by path class ---------------------------------------------------------------------------
def series_finalize(H):
    """k_series_finalize: (passes of its chunk loop, rows of the last pass)."""
    return cdiv(H, C["SS_CHUNK"]), H - (cdiv(H, C["SS_CHUNK"]) - 1) * C["SS_CHUNK"]


def finalize_members(B):
    """k_rollout_finalize: members each of its waves takes (wave w: w, w + 4, ...)."""
    return tuple(len(range(w, B, FIN_WAVES)) for w in range(FIN_WAVES))


def member_blocks(B):
    """Blocks of k_rollout_ws_init, k_rollout_dt, k_ensemble_save_rule, and the live threads of the last one."""
    n = cdiv(B, C["MEMBER_DIV"])
    return n, B - (n - 1) * C["MEMBER_BLOCK"]


def rollout_blocks(H, W):
    """ro_blocks: blocks a member (= partial sums a member) of k_rollout_reduce / k_rollout_step; mc_rollout_blocks exports it."""
    return max(1, min(cdiv(H * W, C["RO_THREADS"]), C["RO_CAP"]))


def walk_lane(W, lane):
    """rs_walk_row: (passes of the four-at-a-time loop, steps of the 64-stride tail) of one lane."""
    j, main, tail = lane, 0, 0
    while j + C["WALK_AHEAD"] < W:
        j, main = j + C["WALK_MAIN"], main + 1
    while j < W:
        j, tail = j + C["WALK_TAIL"], tail + 1
    return main, tail


def walk_row(W):
    return {walk_lane(W, lane) for lane in range(64)}


def walk_columns(W, lane):
    """The columns the lane adds, in the order it adds them."""
    cols, j = [], lane
    while j + C["WALK_AHEAD"] < W:
        cols += [j + C["WALK_LANES"] * q for q in range(C["WALK_QUADS"])]
        j += C["WALK_MAIN"]
    while j < W:
        cols.append(j)
        j += C["WALK_TAIL"]
    return cols


def score_chunks(H):
    """rs_score_row: (chunks of RS_CHUNK rows, rows of the last chunk, waves with no row in the last chunk)."""
    n = cdiv(H, C["RS_CHUNK"])
    last = H - (n - 1) * C["RS_CHUNK"]
    return n, last, max(0, C["RS_WAVES"] - last)


def gather_passes(H, W):
    """k_series_build_input: passes of a thread's grid-stride loop (the most any thread takes)."""
    grid = max(1, min(cdiv(H * W, C["GATHER_THREADS"]), C["GATHER_CAP"]))
    return cdiv(H * W, grid * C["GATHER_BLOCK"])


# ---- the shapes -------------------------------------------------------------------------------------------------------------------
# what the kernel-level tests ran before this table existed (test_eval_seams_host.py holds these against the test files)
OLD_ROLLOUT = [(3, 5, 6), (2, 9, 70), (4, 33, 130), (2, 130, 260)]
OLD_SERIES = [(3, 3, 3), (5, 7, 70), (4, 33, 130)]
OLD_NET_ROLLOUT = [(3, 32, 48), (2, 32, 48)]
OLD_NET_SERIES = [(5, 64, 90)]

# rollout, ensemble statistics, rollout scoring (B, H, W): the path each shape is in the table for
MEMBER_SHAPES = [(257, 5, 5), (6, 9, 70)]
WIDTH_SHAPES = [(2, 5, 250), (2, 5, 506)]
CHUNK_SHAPES = [(2, 128, 5), (2, 129, 5)]
ROLLOUT_PATHS = {
    (257, 5, 5): dict(member_blocks=(2, 1), finalize_members=(65, 64, 64, 64), rollout_blocks=1),
    (6, 9, 70): dict(finalize_members=(2, 2, 1, 1)),
    (2, 5, 250): dict(walk_row={(1, 0), (0, 3)}),                  # lanes 0-57 one main pass; lanes 58-63 three tail steps only
    (2, 5, 506): dict(walk_row={(2, 0), (1, 3)}),                  # the deployed width: lanes 0-57 two main passes
    (2, 128, 5): dict(score_chunks=(1, 128, 0)),
    (2, 129, 5): dict(score_chunks=(2, 1, 15)),
}
# series scoring (N, H, W)
SERIES_SHAPES = [(2, 64, 5), (2, 65, 5), (3, 130, 9)]
GATHER_SHAPE = (1, 513, 520)
SERIES_PATHS = {
    (2, 64, 5): dict(series_finalize=(1, 64)),
    (2, 65, 5): dict(series_finalize=(2, 1)),
    (3, 130, 9): dict(series_finalize=(3, 2)),
    (1, 513, 520): dict(gather_passes=2),
}


def paths(shape):
    """Every path class of a (B or N, H, W)."""
    B, H, W = shape
    return dict(member_blocks=member_blocks(B), finalize_members=finalize_members(B), rollout_blocks=rollout_blocks(H, W),
                walk_row=walk_row(W), score_chunks=score_chunks(H), series_finalize=series_finalize(H), gather_passes=gather_passes(H, W))


# ---- what the GPU tests and the host test share -------------------------------------------------------------------------------------
def grid(H, W):
    xs = np.concatenate(([0.0], (np.arange(W - 2) + 0.5) * 4.0 / (W - 2), [4.0]))
    ys = np.concatenate(([0.0], (np.arange(H - 2) + 0.5) * 1.0 / (H - 2), [1.0]))
    return (np.broadcast_to(xs[None, :], (H, W)).astype(np.float32).copy(), np.broadcast_to(ys[:, None], (H, W)).astype(np.float32).copy())


def rollout_fields(B, H, W):
    """u, v, T [B,H,W] of test_hip_rollout.case: members with different fields; the LAST member is at rest (u = v = 0)."""
    seed = 100 * B + H
    u = fields.smooth_field(B, H, W, seed + 1) * 2000.0
    v = fields.smooth_field(B, H, W, seed + 2) * 2000.0
    u[B - 1] = 0.0
    v[B - 1] = 0.0
    return u, v, fields.temperature_field(B, H, W, seed + 3)


INV = np.array([1.0 / 1700.0, 1.0 / 260.0], dtype=np.float32)       # two simulations, different velocity scales


def series_fields(N, H, W):
    """The host side of test_hip_series_score.case: a store of N snapshots of two simulations (the second half belongs to
    simulation 1) and one prediction per snapshot in the scaled space: the scaled truth plus a smooth error of about 0.1."""
    seed = 1000 * N + H
    u = fields.smooth_field(N, H, W, seed + 1) * 2000.0
    v = fields.smooth_field(N, H, W, seed + 2) * 2000.0
    T = fields.temperature_field(N, H, W, seed + 3)
    sim = np.array([0] * (N - N // 2) + [1] * (N // 2), dtype=np.int32)
    prev = np.full(N, -1, dtype=np.int32)
    for n in range(1, N):
        if sim[n] == sim[n - 1]:
            prev[n] = n - 1
    pred = np.zeros((N, 3, H, W), dtype=np.float32)                  # planes 0, 1 of a 3-channel output: batch stride 3 H W
    pred[:, 0] = u.astype(np.float32) * INV[sim][:, None, None] + fields.smooth_field(N, H, W, seed + 4).astype(np.float32)
    pred[:, 1] = v.astype(np.float32) * INV[sim][:, None, None] + fields.smooth_field(N, H, W, seed + 5).astype(np.float32)
    pred[:, 2] = np.float32("nan")                                    # never read
    return dict(u=u, v=v, T=T, sim=sim, prev=prev, pred=pred)


def member_scalars(B):
    """(vel_scale, RaQ) of the members: the four values the suite has always used; beyond four members, B different values of
    each in an order that is no function of the member's wave (b mod 4) or block (b div 256)."""
    if B <= 4:
        return np.array([0.5, 1.7, 3.0, 0.9])[:B], np.array([1.5, 2.5, 4.0, 9.0])[:B]
    b = np.arange(B)
    return 0.5 + 2.5 * ((97 * b) % B) / B, 1.0 + 8.0 * ((61 * b) % B) / B


def named_members(B):
    """The members the new shapes exist for, by index: the first of a wave's second iteration and its neighbour, the last of
    block 0 and the first of block 1."""
    return [m for m in (4, 5, 255, 256) if m < B]


FROZEN, STEP, LAND = 0, 1, 2


def roles(B, last=None):
    """Who is frozen, who lands, who steps in the stopping tests: member 0 is past its stopping time and member 1 crosses it
    (as ever); beyond four members also 4 (frozen) and 5 (landing); in a second block 253 (landing), 254 (stepping), 255
    (frozen) and the one member of block 1, 256, in the role `last`."""
    r = [STEP] * B
    r[0], r[1] = FROZEN, LAND
    if B > 5:
        r[4], r[5] = FROZEN, LAND
    if B > 256:
        r[253], r[254], r[255] = LAND, STEP, FROZEN
        r[256] = STEP if last is None else last
    return r


# ---- wave-64 sums in numpy f64 ------------------------------------------------------------------------------------------------------
def wave_sum(a):
    """wave_sum_d: a [..., 64] -> what every lane holds after the xor tree (offsets 32, 16, ..., 1)."""
    a = np.asarray(a, np.float64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lanes ^ o]
    return a[..., 0]


def lane_sums(x, order=None, keep=None):
    """x [..., W] -> [..., 64]: lane l adds its columns one after the other from 0.0 (order(W, l): default l, l + 64, ...);
    keep [W] bool: columns a mutant drops."""
    x = np.asarray(x, np.float64)
    W = x.shape[-1]
    out = np.zeros(x.shape[:-1] + (64,))
    for lane in range(64):
        cols = list(range(lane, W, 64)) if order is None else order(W, lane)
        for j in cols:
            if keep is None or keep[j]:
                out[..., lane] = out[..., lane] + x[..., j]
    return out


def ordered(v, chunk, reset=False, maximum=False):
    """v [H] added (maximum: compared) in ascending order, `chunk` rows at a time as the kernels stage them; reset: the mutant
    that loses the running value at every chunk boundary."""
    run = 0.0
    for base in range(0, len(v), chunk):
        if reset:
            run = 0.0
        for x in v[base:base + chunk]:
            run = max(run, float(x)) if maximum else run + float(x)
    return run


# ---- mc_score_rollout in the kernel's order ------------------------------------------------------------------------------------------
SCORE_MUTANTS = ("drop_tail_after_main_lanes_58", "drop_tail_only_lanes", "reset_at_chunk", "bars_first_chunk", "reset_at_one_row_chunk",
                 "bars_without_one_row_chunk")


def score_row_ordered(Tp, Tn, Tr, tau, theta, mutant=None):
    """rs_score_row on host arrays: every sum in the kernel's order.  Returns (row [8], prof [2,H]).  Mutants:
      drop_tail_after_main_lanes_58   lanes >= 58 lose the columns of the tail steps they take after a main pass (W = 506:
                              columns 314 ... 447 of lanes 58-63; no lane >= 58 holds a column >= 448 there)
      drop_tail_only_lanes    the lanes that never enter the four-at-a-time loop lose their columns, in a wave whose other lanes
                              do enter it (W = 250: lanes 58-63)
      reset_at_chunk          the running sums and maxima restart at every chunk boundary
      bars_first_chunk        Abar / Bbar (and prof_mae) from the first chunk only
      reset_at_one_row_chunk, bars_without_one_row_chunk   the same two, only where the last chunk holds ONE row"""
    assert mutant is None or mutant in SCORE_MUTANTS
    a = R.interpolate(Tp, Tn, theta)
    b = np.asarray(Tr, np.float32).astype(np.float64)
    H, W = a.shape
    chunk = C["RS_CHUNK"]
    n_chunks, last_rows, _ = score_chunks(H)
    one_row = n_chunks > 1 and last_rows == 1
    keep = np.ones(W, bool)
    if mutant == "drop_tail_after_main_lanes_58":
        for lane in range(58, 64):
            main, tail = walk_lane(W, lane)
            if main > 0 and tail > 0:
                keep[walk_columns(W, lane)[-tail:]] = False
    if mutant == "drop_tail_only_lanes" and len({m for m, _ in walk_row(W)}) > 1:          # (a wave whose lanes split between the loops)
        keep[[j for j in range(W) if walk_lane(W, j % 64)[0] == 0]] = False
    reset = mutant == "reset_at_chunk" or (mutant == "reset_at_one_row_chunk" and one_row)
    first_only = mutant == "bars_first_chunk" or (mutant == "bars_without_one_row_chunk" and one_row)
    rowsum = lambda x: wave_sum(lane_sums(x, walk_columns, keep))  # noqa: E731
    A, B = rowsum(a) / W, rowsum(b) / W
    bars = (lambda v: ordered(v[:chunk], chunk)) if first_only else (lambda v: ordered(v, chunk, reset))
    Abar, Bbar, pm = bars(A) / H, bars(B) / H, bars(np.abs(A - B)) / H
    d, da, db = np.abs(a - b), a - Abar, b - Bbar
    e1, aa, bb, ab = rowsum(d), rowsum(da * da), rowsum(db * db), rowsum(da * db)
    mx = np.where(keep[None, :], d, 0.0).max(1)
    S = lambda v: ordered(v, chunk, reset)  # noqa: E731
    den = S(aa) * S(bb)
    corr = float("nan") if den == 0.0 else S(ab) / math.sqrt(den)
    row = np.array([tau, theta, S(e1) / (float(H) * float(W)), ordered(mx, chunk, reset, maximum=True), corr, pm, Abar, Bbar])
    return row, np.stack([A, B])


def score_row_passes(row, prof, ref):
    """The comparison of test_hip_rollout_score.check on one row: ref = rollout_score_ref.score_row(...)."""
    return R.within(row, ref["row"], np.nan_to_num(ref["gate"], nan=0.0)) and R.within(prof, ref["prof"], ref["gate_prof"])


def worst_ratio(got, want, gate):
    """max |got - want| / gate over the entries that carry a positive gate."""
    got, want, gate = (np.asarray(x, np.float64) for x in (got, want, gate))
    ok = np.isfinite(want) & np.isfinite(gate) & (gate > 0)
    return float((np.abs(got - want)[ok] / gate[ok]).max()) if ok.any() else 0.0


# ---- mc_series_score / mc_series_score_finalize in the kernels' order ------------------------------------------------------------------
SERIES_MUTANTS = ("first_pass_sums", "acc_restarted", "first_pass_maxima", "profile_first_pass")


def series_rows(uh, vh, ut, vt, ub=None, vb=None):
    """k_series_rows of one item on f64 arrays [H,W] (ut, vt, ub, vb: the scaled f32 products): rows [10,H]."""
    H, W = ut.shape
    eu, ev = np.abs(ut - uh), np.abs(vt - vh)
    z = np.zeros((H, W))
    dp, dt = z.copy(), z.copy()
    dp[1:-1, 1:-1] = np.abs(0.5 * (uh[1:-1, 2:] - uh[1:-1, :-2]) + 0.5 * (vh[2:, 1:-1] - vh[:-2, 1:-1]))
    dt[1:-1, 1:-1] = np.abs(0.5 * (ut[1:-1, 2:] - ut[1:-1, :-2]) + 0.5 * (vt[2:, 1:-1] - vt[:-2, 1:-1]))
    rs = lambda x: wave_sum(lane_sums(x))  # noqa: E731
    nan = np.full(H, np.nan)
    return np.stack([rs(eu), rs(ev), nan if ub is None else rs(np.abs(ut - ub)), nan if vb is None else rs(np.abs(vt - vb)),
                     np.abs(ut).max(1), np.abs(vt).max(1), eu.max(1), ev.max(1), rs(dp), rs(dt)])


def series_finalize_ordered(rows, W, mutant=None):
    """k_series_finalize of one slot: (table [10], profile [2,H]) from rows [10,H].  Mutants:
      first_pass_sums     the six sums stop after the first pass of 64 rows
      acc_restarted       acc restarts at every pass: the table holds the last pass alone
      first_pass_maxima   the four maxima come from the first pass only
      profile_first_pass  profile rows >= 64 stay at the NaN prefill"""
    assert mutant is None or mutant in SERIES_MUTANTS
    H, chunk = rows.shape[1], C["SS_CHUNK"]
    table = np.zeros(10)
    for q in range(10):
        is_max = 4 <= q <= 7
        v = rows[q]
        if (mutant == "first_pass_sums" and not is_max) or (mutant == "first_pass_maxima" and is_max):
            v = v[:chunk]
        acc = ordered(v, chunk, reset=mutant == "acc_restarted", maximum=is_max)
        if q < 4:
            acc = acc / (float(H) * float(W))
        if q >= 8:
            acc = acc / (float(H - 2) * float(W - 2))
        table[q] = acc
    profile = np.stack([rows[0] / float(W), rows[1] / float(W)])
    if mutant == "profile_first_pass":
        profile[:, chunk:] = np.nan
    return table, profile


# ---- mc_ensemble_profiles in the kernel's order ---------------------------------------------------------------------------------------
def profiles_ordered(u, v, s, T):
    """k_ensemble_profiles: prof [B,4,H] with every row's sum taken lane by lane, then the xor tree, then / W."""
    u, v, T = (np.asarray(a).astype(np.float32) for a in (u, v, T))
    s = np.asarray(s).astype(np.float32).reshape(-1, 1, 1)
    su, sv, Td = (s * u).astype(np.float64), (s * v).astype(np.float64), T.astype(np.float64)
    terms = np.stack([Td, su * su, sv * sv, sv * Td], axis=1)
    return wave_sum(lane_sums(terms)) / float(T.shape[-1])


# ---- the per-member kernels: mc_rollout_dt, the clocks of mc_rollout_finalize, the diagnostics --------------------------------------------
MEMBER_MUTANTS = ("partials_of_member_minus_4", "clocks_stop_at_4", "unset_from_256")
CN = 0.1


def diagnostic_terms(Tn, u, v, s, yc):
    """One member, f64 arrays: the summed terms of history columns 2..5 (T_mean, v_rms^2, Nu_bot, Nu_top)."""
    H = Tn.shape[0]
    return {2: Tn.ravel(), 3: ((s * u) ** 2 + (s * v) ** 2).ravel(), 4: (Tn[0, 1:-1] - Tn[1, 1:-1]) / (yc[1, 1:-1] - 0.0),
            5: (Tn[H - 2, 1:-1] - Tn[H - 1, 1:-1]) / (1.0 - yc[H - 2, 1:-1])}


def diagnostics_check(h, Tn, u, v, s, yc, b, rel=1e-6):
    """test_hip_rollout's comparison of one history row h [8] with the member's fields: sums within rel * sum|terms| / count,
    minimum and maximum exactly.  Returns the worst |diff| / gate; raises AssertionError."""
    worst = 0.0
    for col, tm in diagnostic_terms(Tn, u, v, s, yc).items():
        val = h[col] ** 2 if col == 3 else h[col]                # v_rms: the gate is on the mean square it is the root of
        want, gate = tm.sum() / tm.size, rel * np.abs(tm).sum() / tm.size
        print(f"member {b} column {col}: got {val!r} want {want!r} |diff| {abs(val - want):.3e} gate {gate:.3e}")
        assert abs(val - want) <= gate, (b, col, val, want, gate)
        worst = max(worst, abs(val - want) / gate) if gate > 0 else worst
    assert h[6] == Tn.min() and h[7] == Tn.max(), b              # exact
    return worst


def rollout_host(B, H, W, t0=None, t_end=None, steps0=None, mutant=None):
    """One { mc_rollout_dt, mc_rollout_finalize } on the fields of rollout_fields, in numpy: dt (f32 expression of k_rollout_dt),
    flags, the clocks and step counts after the step and the history row whose diagnostics are those of the member's T (the
    field a frozen step copies).  Buffers start from the GPU tests' prefills (dt NaN, flags -1).  Mutants:
      partials_of_member_minus_4  member b >= 4 is given member b - 4's partial sums
      clocks_stop_at_4            clocks and step counters of members >= 4 are not advanced
      unset_from_256              dt / flags of members >= 256 are never written"""
    assert mutant is None or mutant in MEMBER_MUTANTS
    u, v, T = rollout_fields(B, H, W)
    vs, _ = member_scalars(B)
    u32, v32, s32 = u.astype(np.float32), v.astype(np.float32), vs.astype(np.float32)
    xs = grid(H, W)[0]
    dx = np.float32((xs[1:-1, 1:-1] - xs[1:-1, :-2]).min())
    dx2 = dx * dx
    diffusive = np.float32(0.5) * (dx2 * dx2) / (dx2 + dx2)
    t = np.zeros(B) if t0 is None else np.array(t0, np.float64)
    te = np.full(B, np.inf) if t_end is None else np.array(t_end, np.float64)
    steps = np.zeros(B, np.int64) if steps0 is None else np.array(steps0, np.int64)
    dt, flags, hist = np.full(B, np.nan), np.full(B, -1, np.int64), np.full((B, 8), np.nan)
    yc = grid(H, W)[1].astype(np.float64)
    for b in range(B):
        if mutant == "unset_from_256" and b >= 256:
            continue
        su, sv = s32[b] * u32[b, 1:-1, 1:-1], s32[b] * v32[b, 1:-1, 1:-1]
        uv = np.float32(max(np.abs(su).max(), np.abs(sv).max()))
        with np.errstate(divide="ignore"):
            d = min(np.float32(0.5) * np.float32(CN) * dx / uv, diffusive)
        assert isinstance(d, np.float32)
        dd, f = 0.0, FROZEN
        if t[b] < te[b]:
            dd, f = float(d), STEP
            if t[b] + dd >= te[b]:
                dd, f = te[b] - t[b], LAND
        dt[b], flags[b] = dd, f
    for b in range(B):
        if not flags[b] >= 0:
            continue
        tb = te[b] if flags[b] == LAND else (t[b] + dt[b] if flags[b] == STEP else t[b])
        if flags[b] != FROZEN and not (mutant == "clocks_stop_at_4" and b >= 4):
            t[b], steps[b] = tb, steps[b] + 1
        src = b - 4 if (mutant == "partials_of_member_minus_4" and b >= 4) else b
        Tn = T[src].astype(np.float32).astype(np.float64)
        tm = diagnostic_terms(Tn, (s32[src] * u32[src]).astype(np.float64), (s32[src] * v32[src]).astype(np.float64), 1.0, yc)
        hist[b] = [tb, dt[b], tm[2].sum() / tm[2].size, math.sqrt(tm[3].sum() / tm[3].size), tm[4].sum() / tm[4].size,
                   tm[5].sum() / tm[5].size, Tn.min(), Tn.max()]
    return dict(dt=dt, flags=flags, t=t, steps=steps, hist=hist, diffusive=float(diffusive), T=T, u=u32, v=v32, vs=s32, yc=yc)

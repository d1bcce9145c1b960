"""Numpy f64 restatement of mc_score_rollout (include/mantle_hip.h): the crossing rule, the interpolation and the scores of one
row.  Every term is formed in f64 exactly as the kernel forms it (the library is built without contraction, so the terms agree
bit for bit up to the two means they are centred on); every SUM is exactly rounded (math.fsum), so a comparison measures the
kernel's summation error alone.  Beside every quantity the module returns the sum of the magnitudes of the summed terms, and
from those -- never from the kernel's output -- the gates:

  * a quantity that is a sum: depth * 2^-53 * sum|terms|, divided as the quantity is, with
        depth = ceil(W / 64) + 6 + H + 8
    = the additions one value passes through in the prescribed order (a lane's ceil(W/64) columns, the 6 levels of the xor
    tree, at most H rows added in ascending order) plus 8 for the roundings inside one term (difference, product with theta,
    sum, centring, square, the division).  Derived, not measured.
      - the row means A_i, B_i: the terms are the row's a (b);
      - T_mean_pred, T_mean_true, mae, Saa, Sbb, Sab: the terms are the cells' a, b, |a-b|, (a-Abar)^2, (b-Bbar)^2, (a-Abar)(b-Bbar);
      - prof_mae = sum_i |A_i - B_i| / h: each A_i - B_i is itself a difference of two sums, so its summed terms are the cells'
        a AND b: sum|terms| = sum|a| + sum|b|, divided by h w.
  * corr = Sab / sqrt(Saa Sbb): that relative bound on Saa and Sbb (positive terms: depth * 2^-53 each) and on Sab with its own
    condition number sum|terms| / |sum terms|, propagated through the quotient: rel = rel(Sab) + (rel(Saa) + rel(Sbb)) / 2,
    plus 4 ulp for the product, the root and the division.
  * max_err, theta and t: 4 ulp each."""
import math

import numpy as np

FROZEN, STEP, LAND = 0, 1, 2
NAMES = ("t", "theta", "mae", "max_err", "corr", "prof_mae", "T_mean_pred", "T_mean_true")
U = 2.0 ** -53


def depth(H, W):
    return -(-W // 64) + 6 + H + 8


def ulp4(x):
    return 4.0 * float(np.spacing(abs(np.float64(x))))


def end_of_step(flag, t0, dt, t_end):
    """The clock mc_rollout_finalize will store."""
    t0 = np.float64(t0)
    if flag == LAND:
        return np.float64(t_end)
    if flag == STEP:
        return t0 + np.float64(dt)
    return t0


def crossing(flag, t0, t1, times, n, capacity, k):
    """The while rule for one member: ([(row, tau, theta)] to score, skipped count, next)."""
    due, skipped = [], 0
    if flag == FROZEN:
        return due, skipped, int(k)
    t0, t1, k = np.float64(t0), np.float64(t1), int(k)
    while k < min(int(n), int(capacity)) and np.float64(times[k]) <= t1:
        tau = np.float64(times[k])
        if tau < t0:
            skipped += 1
        else:
            due.append((k, tau, (tau - t0) / (t1 - t0) if t1 > t0 else np.float64(0.0)))
        k += 1
    return due, skipped, k


def interpolate(Tp, Tn, theta):
    Tp, Tn = np.asarray(Tp, np.float32).astype(np.float64), np.asarray(Tn, np.float32).astype(np.float64)
    return Tp + np.float64(theta) * (Tn - Tp)


def score_row(Tp, Tn, Tr, tau, theta):
    """Scores of one truth snapshot: dict(row [8], prof [2,H], gate [8], gate_prof [2,H], mag {name: sum|terms|})."""
    a = interpolate(Tp, Tn, theta)
    b = np.asarray(Tr, np.float32).astype(np.float64)
    H, W = a.shape
    D = depth(H, W) * U
    A = np.array([math.fsum(r) / W for r in a])
    B = np.array([math.fsum(r) / W for r in b])
    magA, magB = np.abs(a).sum(1), np.abs(b).sum(1)
    Abar, Bbar = math.fsum(A) / H, math.fsum(B) / H
    e = np.abs(a - b)
    da, db = a - Abar, b - Bbar
    saa, sbb, sab = da * da, db * db, da * db
    Saa, Sbb, Sab = math.fsum(saa.ravel()), math.fsum(sbb.ravel()), math.fsum(sab.ravel())
    mae, max_err = math.fsum(e.ravel()) / (H * W), float(e.max())
    prof_mae = math.fsum(np.abs(A - B)) / H
    den = Saa * Sbb
    corr = float("nan") if den == 0.0 else Sab / math.sqrt(den)
    mag = dict(mae=float(e.sum()), Saa=float(saa.sum()), Sbb=float(sbb.sum()), Sab=float(np.abs(sab).sum()),
               prof_mae=float(magA.sum() + magB.sum()), T_mean_pred=float(magA.sum()), T_mean_true=float(magB.sum()))
    if den == 0.0 or Sab == 0.0:
        g_corr = float("nan") if den == 0.0 else D * mag["Sab"] / math.sqrt(den) + ulp4(1.0)
    else:
        g_corr = abs(corr) * (D * mag["Sab"] / abs(Sab) + 0.5 * (D + D)) + ulp4(corr)
    row = np.array([tau, theta, mae, max_err, corr, prof_mae, Abar, Bbar], dtype=np.float64)
    gate = np.array([ulp4(tau), ulp4(theta), D * mag["mae"] / (H * W), ulp4(max_err), g_corr, D * mag["prof_mae"] / (H * W),
                     D * mag["T_mean_pred"] / (H * W), D * mag["T_mean_true"] / (H * W)], dtype=np.float64)
    return dict(row=row, prof=np.stack([A, B]), gate=gate, gate_prof=np.stack([D * magA / W, D * magB / W]), mag=mag,
                sums=dict(Saa=Saa, Sbb=Sbb, Sab=Sab))


def step(T_prev, T_next, t, dt, flags, t_end, truth, truth_t, n_truth, capacity, nxt, scored, skipped, table, prof):
    """One call of mc_score_rollout on host arrays.  Returns copies: dict(next, scored, skipped, table [b,cap,8], prof
    [b,cap,2,h], gate (NaN where nothing was written), gate_prof, rows = [(m, k)] written)."""
    b = len(flags)
    nxt, scored, skipped = (np.array(x, dtype=np.int64).copy() for x in (nxt, scored, skipped))
    table, prof = np.array(table, dtype=np.float64).copy(), np.array(prof, dtype=np.float64).copy()
    gate, gate_prof, rows = np.full_like(table, np.nan), np.full_like(prof, np.nan), []
    for m in range(b):
        t1 = end_of_step(int(flags[m]), t[m], dt[m], t_end[m])
        due, sk, k = crossing(int(flags[m]), t[m], t1, truth_t[m], n_truth[m], capacity, nxt[m])
        for (r, tau, theta) in due:
            s = score_row(T_prev[m], T_next[m], truth[m][r], tau, theta)
            table[m, r], prof[m, r], gate[m, r], gate_prof[m, r] = s["row"], s["prof"], s["gate"], s["gate_prof"]
            rows.append((m, r))
        nxt[m], scored[m], skipped[m] = k, scored[m] + len(due), skipped[m] + sk
    return dict(next=nxt, scored=scored, skipped=skipped, table=table, prof=prof, gate=gate, gate_prof=gate_prof, rows=rows)


def within(got, want, gate):
    """Elementwise |got - want| <= gate, a NaN expected where (and only where) a NaN is wanted."""
    got, want, gate = (np.asarray(x, dtype=np.float64) for x in (got, want, gate))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)) and bool((np.abs(got - want)[~nan] <= gate[~nan]).all())

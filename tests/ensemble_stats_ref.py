"""numpy f64 restatement of the ensemble rollout's statistics (mc_ensemble_profiles, mc_ensemble_snapshot): the time weight
of a step, the depth profiles of one state and the save rule on a member's own clock.  Shared by the host and GPU tests."""
import numpy as np

FROZEN, STEP, LAND = 0, 1, 2


def time_weight(flag, t0, d, ta):
    """Weight of the step that starts at t0 and takes d, averaging from ta on: a left Riemann sum (f64 arithmetic)."""
    t0, d, ta = np.float64(t0), np.float64(d), np.float64(ta)
    if int(flag) == FROZEN:
        return np.float64(0.0)
    return d if ta <= t0 else np.float64(max(0.0, (t0 + d) - ta))


def profiles(u, v, s, T):
    """u, v, T [B,H,W] and s [B] hold float32 values.  s*u and s*v are single float32 products; squares, products and sums
    are f64.  Returns (prof [B,4,H], abs_sum [B,4,H]): the means over ALL W columns of (T, (su)^2, (sv)^2, (sv) T) and the
    sums of the terms' magnitudes that the gate 1e-12 * abs_sum / W is built from."""
    u, v, T = (np.asarray(a).astype(np.float32) for a in (u, v, T))
    s = np.asarray(s).astype(np.float32).reshape(-1, 1, 1)
    su, sv, Td = (s * u).astype(np.float64), (s * v).astype(np.float64), T.astype(np.float64)
    assert (s * u).dtype == np.float32
    terms = np.stack([Td, su * su, sv * sv, sv * Td], axis=1)               # [B,4,H,W]
    W = T.shape[-1]
    return terms.sum(-1) / W, np.abs(terms).sum(-1)


def save_rule(clocks, flags, save_every, capacity, next_save=0.0):
    """One member: clocks[k] is its clock after step k + 1, flags[k] that step's flag.  The reference loop's
    `if t > save_t: save_t = t + save_every` with `capacity` slots.  Returns (steps saved into slots (0-based), steps missed,
    next_save after the last step)."""
    nxt, saved, missed = np.float64(next_save), [], []
    for k, (t, f) in enumerate(zip(clocks, flags)):
        t = np.float64(t)
        if int(f) != FROZEN and save_every > 0 and t > nxt:
            (saved if len(saved) < capacity else missed).append(k)
            nxt = t + np.float64(save_every)
    return saved, missed, nxt

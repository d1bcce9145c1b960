"""numpy restatement of the series-scoring contract (mc_series_score, mc_series_score_finalize): the same single f32 products
u * inv_scale, f64 everywhere else.  Shared by the host and GPU tests."""
import numpy as np

NAMES = ("mae_u", "mae_v", "base_u", "base_v", "max_u", "max_v", "maxerr_u", "maxerr_v", "mass_pred", "mass_true")
SUM_COLS, MAX_COLS = (0, 1, 2, 3, 8, 9), (4, 5, 6, 7)


def div_abs(a, b):
    """|div(a, b)| on interior rows and columns, a, b [H,W] f64: get_mass(..., bc=False)."""
    return np.abs(0.5 * (a[1:-1, 2:] - a[1:-1, :-2]) + 0.5 * (b[2:, 1:-1] - b[:-2, 1:-1]))


def scaled(x, inv):
    """One f32 product, then f64."""
    p = np.asarray(x, dtype=np.float32) * np.float32(inv)
    assert p.dtype == np.float32
    return p.astype(np.float64)


def score(u_hat, v_hat, u, v, sim, prev, inv_scale, idx):
    """u_hat, v_hat [n,H,W] f32: the network's planes of item j (snapshot idx[j]); u, v [N,H,W] f32, sim, prev [N], inv_scale
    [S] f32.  Returns (table [n,10], profile [n,2,H], gate_table [n,10], gate_profile [n,2,H]); the gates are 1e-12 * sum|terms| /
    count for the sums and 0 for the four maxima, which are exact."""
    idx = np.asarray(idx).reshape(-1)
    n = idx.shape[0]
    H, W = u.shape[-2:]
    table, gate = np.zeros((n, 10)), np.zeros((n, 10))
    profile, pgate = np.zeros((n, 2, H)), np.zeros((n, 2, H))
    for j, s in enumerate(idx.tolist()):
        inv = np.float32(inv_scale[int(sim[s])])
        ut, vt = scaled(u[s], inv), scaled(v[s], inv)
        uh, vh = np.asarray(u_hat[j], dtype=np.float32).astype(np.float64), np.asarray(v_hat[j], dtype=np.float32).astype(np.float64)
        eu, ev = np.abs(ut - uh), np.abs(vt - vh)
        sums = {0: eu.sum(), 1: ev.sum(), 8: div_abs(uh, vh).sum(), 9: div_abs(ut, vt).sum()}
        if prev[s] >= 0:
            ub, vb = scaled(u[int(prev[s])], inv), scaled(v[int(prev[s])], inv)
            sums[2], sums[3] = np.abs(ut - ub).sum(), np.abs(vt - vb).sum()
        else:
            sums[2] = sums[3] = np.nan
        for q in SUM_COLS:
            count = (H - 2) * (W - 2) if q >= 8 else H * W
            table[j, q] = sums[q] / count
            gate[j, q] = 0.0 if np.isnan(sums[q]) else 1e-12 * sums[q] / count        # the terms are non-negative: sum|terms| = sum
        table[j, 4:8] = np.abs(ut).max(), np.abs(vt).max(), eu.max(), ev.max()
        profile[j, 0], profile[j, 1] = eu.sum(-1) / W, ev.sum(-1) / W
        pgate[j, 0], pgate[j, 1] = 1e-12 * eu.sum(-1) / W, 1e-12 * ev.sum(-1) / W
    return table, profile, gate, pgate


def close(got, want, gate):
    """NaN where NaN is wanted, elsewhere |got - want| <= gate."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and bool((np.abs(got - want)[~nan] <= np.asarray(gate)[~nan]).all())

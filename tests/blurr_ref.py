"""f64 reference, case tables, derived bounds, comparison functions and mutants for the blurred-streamfunction heads of
csrc/curl_head.hip (`-blurr 1`: mc_curl_blur_head_* and mc_curl_blur_valid_*; tests/test_hip_blurr.py and
tests/test_hip_blurr_net.py on the GPU, tests/test_blurr_ref_host.py on the CPU).

Definition (reference pytorch_networks_convae.py:1357-1388 and :1682-1697).  A = a_bound * y[:, 0] on the Hp x Wp plane the head
reads (H x W for NewFluidNet's wall form, (H+2) x (W+2) for FluidNet's valid form),

    B[i][j] = w * sum_{di, dj in {-1,0,1}} A[clamp(i+di, 0, Hp-1)][clamp(j+dj, 0, Wp-1)],    w = float32(1) / float32(9),

u_in = 0.5 (B[i+2][j+1] - B[i][j+1]) and v_in = -0.5 (B[i+1][j+2] - B[i+1][j]) on (Hp-2) x (Wp-2).  The valid form returns
u_in, v_in; the wall form pads them by one (replicate), negates the wall columns of u and the wall rows of v and zeroes the
corners.  The adjoints below are written as the literal transposes (scatter + fold), independently of the forward's gathers.

Bounds.  U = 2^-24.  Every bound is K x U x (the reference with every addend replaced by its magnitude: `mag=True`), with K the
number of roundings on the longest chain of the kernel's expression (-ffp-contract=off: every operation rounds once):

  K_FWD = 7        k_curl_blur_fwd: the middle row (column) of the two box sums cancels, twelve taps remain per component:
                   d1 = A[+2] - A[-2] (1), d2 = A[+1] - A[-1] (1, parallel), s = d1 + d2 (2) per column (row) of the box,
                   (s0 + s1) (3), + s2 (4), k = a_bound (0.5 w) (one rounding of its own: 0.5 w is exact) (5), k x sum (6);
                   the f32 store is exact, one in hand (7)
  K_BWD_VALID = 10 k_curl_blur_bwd: gB = ((eu[r-2] - eu[r]) - ev[c-2]) + ev[c] (3), the row sums (g[c-1] + g[c]) + g[c+1] (5),
                   (t0 + t1) + t2 (7), k (8), k x sum (9), one in hand (10)
  K_BWD_WALL = 14  the same gather after k_curl_bwd_fold, whose sums hold at most five terms (h = 3 or w = 3: the pixel's own
                   value, two walls, and no corner): four roundings more
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

f64 = torch.float64
U = 2.0 ** -24
W32 = float(np.float32(1.0) / np.float32(9.0))           # the reference's torch.Tensor([[1 / 9] * 3] * 3), widened
K_FWD, K_BWD_VALID, K_BWD_WALL = 7, 10, 14

# tile of csrc/curl_head.hip's blurred kernels (BT_Y x BT_X outputs per block), restated
BT_Y, BT_X = 16, 64
N, CC = 2, 3                                              # batch, channels of y (the batch stride leaves a two-plane gap)
AB_WALL, AB_VALID = 4.0, 10.0                             # NewFluidNet's default a_bound, the FluidNet run list's
# wall form (h, w): the minimum (all wall or corner); the smallest interior that clamps on one side only; one-wide interiors
# beyond a wave of columns / rows; one past the tile's width, its height, and both; several tiles with a ragged last one
WALL_SHAPES = [(3, 3), (4, 4), (3, 70), (40, 3), (4, BT_X + 1), (BT_Y + 1, 4), (BT_Y + 1, BT_X + 1), (35, 300)]
# valid form (h, w) of u, v (the plane is (h+2) x (w+2)): the same set with the degenerate ones, and (BT_Y - 1, BT_X - 1),
# whose PLANE is one past the tile (the adjoint's tiles cover the plane)
VALID_SHAPES = [(1, 1), (4, 4), (1, 70), (40, 1), (4, BT_X + 1), (BT_Y + 1, 4), (BT_Y + 1, BT_X + 1), (BT_Y - 1, BT_X - 1),
                (35, 300)]
MUTANTS = ("zero_pad", "w8", "adj_ny1", "blur_after")


def t64(a):
    return a.to(f64) if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def case(form, h, w):
    """Seeded f32 inputs of one shape: y [N, CC, hp, wp] (channel 0 = streamfunction), gu, gv [N, h, w]."""
    g = 2 if form == "valid" else 0
    rng = np.random.RandomState(7919 * h + w + (1 if form == "valid" else 0))
    return dict(form=form, h=h, w=w, ab=AB_VALID if form == "valid" else AB_WALL,
                y=rng.standard_normal((N, CC, h + g, w + g)).astype(np.float32),
                gu=rng.standard_normal((N, h, w)).astype(np.float32), gv=rng.standard_normal((N, h, w)).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ the blur
def _weights(variant):
    w = 1.0 / 9.0 if variant == "w64" else W32
    wt = [[w] * 3 for _ in range(3)]
    if variant == "w8":                                    # mutant: 1/8 on the eight outer taps
        wt = [[0.125] * 3 for _ in range(3)]
        wt[1][1] = w
    return wt


def box_mean(A, variant=None):
    """B of the definition on the last two dimensions (by clamped index; `zero_pad`: taps outside the plane read 0)."""
    A = t64(A)
    Hp, Wp = A.shape[-2:]
    wt = _weights(variant)
    B = torch.zeros_like(A)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            r, c = torch.arange(Hp) + di, torch.arange(Wp) + dj
            T = A[..., r.clamp(0, Hp - 1), :][..., c.clamp(0, Wp - 1)]
            if variant == "zero_pad":
                T = T * ((r >= 0) & (r < Hp)).to(f64)[:, None] * ((c >= 0) & (c < Wp)).to(f64)[None, :]
            B = B + wt[di + 1][dj + 1] * T
    return B


def box_mean_T(G, variant=None):
    """The transpose of box_mean: scatter every G[r'][c'] to its nine taps on the padded plane, then fold the pad's ring onto
    the rows and columns it replicates: ny(0, 0) = 2.  (`adj_ny1` and `zero_pad` drop the ring instead.)"""
    G = t64(G)
    Hp, Wp = G.shape[-2:]
    wt = _weights(variant)
    E = torch.zeros(G.shape[:-2] + (Hp + 2, Wp + 2), dtype=f64)
    for di in (0, 1, 2):
        for dj in (0, 1, 2):
            E[..., di:di + Hp, dj:dj + Wp] += wt[di][dj] * G
    if variant not in ("adj_ny1", "zero_pad"):
        E[..., 1, :] += E[..., 0, :]
        E[..., -2, :] += E[..., -1, :]
        E[..., :, 1] += E[..., :, 0]
        E[..., :, -2] += E[..., :, -1]
    return E[..., 1:-1, 1:-1].clone()


# --------------------------------------------------------------------------------------------------------------- the stencils
def _diffs(B, mag):
    s = 1.0 if mag else -1.0
    return 0.5 * (B[..., 2:, 1:-1] + s * B[..., :-2, 1:-1]), (0.5 if mag else -0.5) * (B[..., 1:-1, 2:] + s * B[..., 1:-1, :-2])


def _diffs_T(eu, ev, mag):
    """gB [.., hp, wp] from the gradients w.r.t. u_in, v_in [.., hp-2, wp-2]."""
    s = 1.0 if mag else -1.0
    G = torch.zeros(eu.shape[:-2] + (eu.shape[-2] + 2, eu.shape[-1] + 2), dtype=f64)
    G[..., 2:, 1:-1] += 0.5 * eu
    G[..., :-2, 1:-1] += s * 0.5 * eu
    G[..., 1:-1, 2:] += s * 0.5 * ev
    G[..., 1:-1, :-2] += 0.5 * ev
    return G


def _wall(u_in, v_in, mag):
    """Replicate pad by one, antisymmetric wall columns of u / wall rows of v, zero corners."""
    s = 1.0 if mag else -1.0
    shape = tuple(u_in.shape[:-2]) + (u_in.shape[-2] + 2, u_in.shape[-1] + 2)
    u = F.pad(u_in.reshape((-1, 1) + tuple(u_in.shape[-2:])), (1, 1, 1, 1), mode="replicate").reshape(shape).clone()
    v = F.pad(v_in.reshape((-1, 1) + tuple(v_in.shape[-2:])), (1, 1, 1, 1), mode="replicate").reshape(shape).clone()
    u[..., :, 0] *= s
    u[..., :, -1] *= s
    v[..., 0, :] *= s
    v[..., -1, :] *= s
    for t in (u, v):
        for i in (0, -1):
            for j in (0, -1):
                t[..., i, j] = 0.0
    return u, v


def _wall_T(gu, gv, mag):
    """(eu, ev) [.., h-2, w-2]: the transpose of _wall (what k_curl_bwd_fold computes)."""
    s = 1.0 if mag else -1.0
    gu, gv = gu.clone(), gv.clone()
    gu[..., :, 0] *= s
    gu[..., :, -1] *= s
    gv[..., 0, :] *= s
    gv[..., -1, :] *= s
    out = []
    for g in (gu, gv):
        for i in (0, -1):
            for j in (0, -1):
                g[..., i, j] = 0.0
        r = g[..., 1:-1, :].clone()                         # fold the replicated rows, then the columns
        r[..., 0, :] += g[..., 0, :]
        r[..., -1, :] += g[..., -1, :]
        c = r[..., :, 1:-1].clone()
        c[..., :, 0] += r[..., :, 0]
        c[..., :, -1] += r[..., :, -1]
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------ the heads
def head(form, y0, ab, variant=None, mag=False):
    """(u, v) of a head from the streamfunction channel y0 [.., hp, wp] (torch f64; differentiable).  mag: every addend by its
    magnitude.  variant: a mutant, or 'w64' (the weight 1/9 in f64)."""
    A = ab * t64(y0)
    if mag:
        A = A.abs()
    if variant == "blur_after":                             # mutant: the mean of the finished u, v instead of the streamfunction's
        u, v = _diffs(A, mag)
        if form == "wall":
            u, v = _wall(u, v, mag)
        return box_mean(u), box_mean(v)
    u, v = _diffs(box_mean(A, variant), mag)
    return _wall(u, v, mag) if form == "wall" else (u, v)


def head_adj(form, gu, gv, ab, variant=None, mag=False):
    """ga [.., hp, wp] = d(<u, gu> + <v, gv>) / d y0, as the transposes applied in reverse order."""
    gu, gv = t64(gu), t64(gv)
    if mag:
        gu, gv = gu.abs(), gv.abs()
    if variant == "blur_after":
        gu, gv = box_mean_T(gu), box_mean_T(gv)
    eu, ev = _wall_T(gu, gv, mag) if form == "wall" else (gu, gv)
    G = _diffs_T(eu, ev, mag)
    return ab * (G if variant == "blur_after" else box_mean_T(G, variant))


def head_conv2d(form, y0, ab):
    """The reference's own expression (F.pad replicate, F.conv2d with the widened f32 filter, then its differences and wall
    rules), for the restatement check and, through autograd, for the adjoint."""
    a = (ab * t64(y0)).reshape((-1, 1) + tuple(y0.shape[-2:]))
    a = F.conv2d(F.pad(a, (1, 1, 1, 1), mode="replicate"), torch.tensor([[W32] * 3] * 3, dtype=f64).view(1, 1, 3, 3))
    ky = torch.tensor([-0.5, 0.0, 0.5], dtype=f64).view(1, 1, 3, 1)
    kx = torch.tensor([-0.5, 0.0, 0.5], dtype=f64).view(1, 1, 1, 3)
    u = F.conv2d(a, ky)[:, :, :, 1:-1]
    v = -F.conv2d(a, kx)[:, :, 1:-1, :]
    if form == "wall":
        u = F.pad(u, (1, 1, 1, 1), mode="replicate")
        v = F.pad(v, (1, 1, 1, 1), mode="replicate")
        mu, mv = torch.ones_like(u), torch.ones_like(v)
        mu[..., :, 0] = mu[..., :, -1] = -1.0
        mv[..., 0, :] = mv[..., -1, :] = -1.0
        for m in (mu, mv):
            m[..., 0, 0] = m[..., 0, -1] = m[..., -1, 0] = m[..., -1, -1] = 0.0
        u, v = u * mu, v * mv
    shape = tuple(y0.shape[:-2])
    return u.reshape(shape + tuple(u.shape[-2:])), v.reshape(shape + tuple(v.shape[-2:]))


# ----------------------------------------------------------------------------------------------------------------- comparisons
def ratio(got, ref, bound):
    """The largest |got - ref| / bound; where the bound is 0 (the corners: no addend at all) the value must be exactly 0."""
    got, ref, bound = (np.asarray(t.detach().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float("inf")
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def fwd_ratio(c, u, v):
    """Worst err / bound of a forward result (u, v) [N, h, w] on case c."""
    ru, rv = head(c["form"], c["y"][:, 0], c["ab"])
    mu, mv = head(c["form"], c["y"][:, 0], c["ab"], mag=True)
    return max(ratio(u, ru, K_FWD * U * mu), ratio(v, rv, K_FWD * U * mv))


def bwd_ratio(c, ga):
    """Worst err / bound of an adjoint result ga [N, hp, wp] on case c."""
    K = K_BWD_WALL if c["form"] == "wall" else K_BWD_VALID
    return ratio(ga, head_adj(c["form"], c["gu"], c["gv"], c["ab"]), K * U * head_adj(c["form"], c["gu"], c["gv"], c["ab"], mag=True))


def identity_ratio(c, u, v, ga):
    """|<u, gu> + <v, gv> - <y0, ga>| in f64 of the given results over the sum of their bounds."""
    K = K_BWD_WALL if c["form"] == "wall" else K_BWD_VALID
    y0, gu, gv = t64(c["y"][:, 0]), t64(c["gu"]), t64(c["gv"])
    mu, mv = head(c["form"], y0, c["ab"], mag=True)
    mg = head_adj(c["form"], gu, gv, c["ab"], mag=True)
    lhs = float((t64(u) * gu).sum() + (t64(v) * gv).sum())
    rhs = float((y0 * t64(ga)).sum())
    tol = float(K_FWD * U * ((mu * gu.abs()).sum() + (mv * gv.abs()).sum()) + K * U * (mg * y0.abs()).sum())
    return abs(lhs - rhs) / tol


def close64(a, b, rel=1e-12):
    """Agreement at f64 tolerance: max |a - b| <= rel max |b| (the restatement agrees with the reference to 2e-14 of max |u|;
    the f64 weight 1/9 is off by 7e-9)."""
    a, b = (np.asarray(t.detach().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (a, b))
    return a.shape == b.shape and float(np.abs(a - b).max()) <= rel * float(np.abs(b).max())


def golden_parts(g, u, v):
    """[(got, want)] of complete fields u, v [1, H, W] against what a g25 file stores: strided samples and the edges."""
    import fields
    out = []
    for n, o in (("u", u), ("v", v)):
        o = np.asarray(o.detach().numpy() if isinstance(o, torch.Tensor) else o)
        out.append((fields.strided_sample(o, 5003), g["out/" + n]))
        out += [(o[:, :2], g[f"edge/{n}/top"]), (o[:, -2:], g[f"edge/{n}/bottom"]), (o[:, :, :2], g[f"edge/{n}/left"]),
                (o[:, :, -2:], g[f"edge/{n}/right"])]
    return out

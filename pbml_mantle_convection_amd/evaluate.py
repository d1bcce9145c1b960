"""Series scoring: a trained Stokes net against the snapshots of a simulation, on the device (DESIGN.md §9 "Series scoring").

What the reference does in load_fluidnet.ipynb one snapshot at a time -- TS without an advection net, truth and prediction
scaled with scale_var, MAE of u and v, the same MAE of the "baseline" (the previous snapshot taken as the prediction), the
largest error beside max|truth| and the mass residual of prediction and truth -- for a whole store of snapshots: one scoring
step = input gather -> NewFluidNet -> row pass -> finalize, captured as ONE HIP graph of fixed batch and replayed over a work
list with no host synchronisation inside the loop.

    python -m pbml_mantle_convection_amd.evaluate --weights sd.pt -l 5 -f 16 -r 6 -k 5 -p zeros --data_dir DIR --an cv \
        [--sims 3 7] [--every 1] [--batch 32] [--precision bf16] [--graph 1] --out DIR
    python -m pbml_mantle_convection_amd.evaluate --synthetic 64 128 506 --out DIR        # seeded fields instead of files

Rollout scoring (DESIGN.md §9 "Rollout scoring"): with --rollout_steps N the coupled loop (net + advection-diffusion step) of
the checkpoint starts from snapshot --start of every selected simulation and is scored against the later snapshots at their
own simulated times (times.pt) by rollout.EnsembleRollout(score_capacity=...):

    python -m pbml_mantle_convection_amd.evaluate --weights sd.pt ... --data_dir DIR --an cv --rollout_steps 5000 \
        [--start 0] [--truth_every 10] [--truth_count 16] [--t_end X] --out DIR
"""
import argparse
import csv
import json
import os

import numpy as np
import torch

from . import _lib as L
from .datasetio import _GridMixin, _load, _selected_sims
from .rollout import SCORE_NAMES as ROLLOUT_SCORE_NAMES
from .rollout import EnsembleRollout, build_stokes, normalise_params, synthetic_ensemble
from .scaler import velocity_scaler

SCORE_NAMES = ("mae_u", "mae_v", "base_u", "base_v", "max_u", "max_v", "maxerr_u", "maxerr_v", "mass_pred", "mass_true")


def inverse_velocity_scale(raq, fkt, fkp):
    """1 / scaler.velocity_scaler per simulation: evaluated in f64, rounded ONCE to f32 (the factor of the kernels' single f32
    product u * inv_scale)."""
    r, t, p = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (raq, fkt, fkp))
    return (1.0 / velocity_scaler(r, t, p)).astype(np.float32)


def previous_snapshots(sim):
    """prev[n] = the preceding snapshot of the same simulation in store order, -1 for a simulation's first."""
    sim = np.asarray(sim).reshape(-1)
    prev = np.full(sim.shape[0], -1, dtype=np.int32)
    last = {}
    for n, s in enumerate(sim.tolist()):
        prev[n] = last.get(s, -1)
        last[s] = n
    return prev


class SeriesStore:
    """N snapshots on ONE mesh, f32 on the device: T, u, v [N,H,W] un-scaled as the files hold them; sim [N] (row of the
    parameter arrays the snapshot belongs to), prev [N] (index of its baseline snapshot, -1 = none); per simulation paras [S,3] =
    (RaQ, FKT, FKP), nd [S,3] (rollout.normalise_params) and inv_scale [S] (inverse_velocity_scale).  Host arrays in."""

    def __init__(self, T, u, v, sim, prev, raq, fkt, fkp, xc, yc, ycc=None, device="cuda:0", sim_ids=None):
        self.device = device if isinstance(device, torch.device) else torch.device(device)
        xc = np.asarray(xc, dtype=np.float32)
        H, W = xc.shape[-2:]
        if H < 3 or W < 3:
            raise ValueError("the grid must be at least 3 x 3")
        field = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, H, W))  # noqa: E731
        T, u, v = field(T), field(u), field(v)
        N = T.shape[0]
        if N == 0 or u.shape[0] != N or v.shape[0] != N:
            raise ValueError(f"T, u and v must hold the same, positive number of snapshots, got {T.shape[0]}, {u.shape[0]}, {v.shape[0]}")
        paras = np.stack([np.asarray(a, dtype=np.float64).reshape(-1) for a in (raq, fkt, fkp)], axis=1)
        S = paras.shape[0]
        if S == 0 or (paras[:, 1:] <= 0).any():
            raise ValueError("raq, fkt, fkp must hold one row per simulation, fkt and fkp positive")
        sim = np.asarray(sim, dtype=np.int64).reshape(-1)
        prev = np.asarray(prev, dtype=np.int64).reshape(-1)
        if sim.shape[0] != N or prev.shape[0] != N:
            raise ValueError(f"sim and prev must hold one entry per snapshot ({N})")
        if sim.min() < 0 or sim.max() >= S:
            raise ValueError(f"sim must index the {S} parameter rows")
        if prev.min() < -1 or prev.max() >= N:
            raise ValueError(f"prev must be -1 or index the {N} snapshots")
        plane = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, H, W)[0])  # noqa: E731
        dev = self.device
        put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev).contiguous()  # noqa: E731
        f32, i32 = torch.float32, torch.int32
        self.N, self.S, self.H, self.W = N, S, H, W
        self.T, self.u, self.v = put(T, f32), put(u, f32), put(v, f32)
        self.sim, self.prev = put(sim, i32), put(prev, i32)
        self.paras, self.nd = put(paras, f32), put(normalise_params(paras), f32)
        self.inv_scale = put(inverse_velocity_scale(paras[:, 0], paras[:, 1], paras[:, 2]), f32)
        self.xc, self.yc = put(plane(xc), f32), put(plane(yc), f32)
        self.ycc = put(plane(yc if ycc is None else ycc), f32)
        self.sim_ids = list(range(S)) if sim_ids is None else [int(s) for s in sim_ids]

    TENSORS = ("T", "u", "v", "sim", "prev", "paras", "nd", "inv_scale", "xc", "yc", "ycc")

    def shape(self):
        return (self.N, self.S, self.H, self.W)


class _Grid(_GridMixin):
    pass


def load_series(data_dir, an, sims=None, every=1):
    """Host arrays of the full series of the simulations of split `an` in the reference's layout (`sims.pt`,
    `<an>/sim_<n>/xc.pt`, `yc.pt`, `e1_{u,v,T}prev_data.pt`), every `every`-th snapshot, `sims` = simulation numbers (None =
    all of the split).  The mesh is loaded the way the datasets load it (wall coordinates written into the first / last row
    and column), so it is the mesh training saw.  prev is the preceding KEPT snapshot of the same simulation.  Returns a dict
    of SeriesStore's arguments: SeriesStore(**load_series(...), device=dev)."""
    every = int(every)
    if every < 1:
        raise ValueError("every must be at least 1")
    want = None if sims is None else {int(s) for s in sims}
    T, u, v, sim, raq, fkt, fkp, ids = [], [], [], [], [], [], [], []
    xc = yc = None
    for entry, d in _selected_sims(str(data_dir), an):
        if want is not None and int(entry[0]) not in want:
            continue
        g = _Grid()
        g._load_grid(d)
        gx, gy = g.xc[0].numpy(), g.yc[0].numpy()
        if xc is None:
            xc, yc = gx, gy
        elif gx.shape != xc.shape or not (np.array_equal(gx, xc) and np.array_equal(gy, yc)):
            raise ValueError(f"a store holds one depth grid: simulation {entry[0]} lies on another mesh than simulation {ids[0]}")
        H, W = xc.shape
        Ts, us, vs = (_load(d + f"/e1_{k}prev_data.pt").reshape(-1, H, W)[::every].float().numpy() for k in "Tuv")
        if not (Ts.shape[0] == us.shape[0] == vs.shape[0]):
            raise ValueError(f"{d}: T, u and v hold different numbers of snapshots")
        T.append(Ts); u.append(us); v.append(vs)
        sim.append(np.full(Ts.shape[0], len(ids), dtype=np.int32))
        raq.append(float(entry[2])); fkt.append(float(entry[3])); fkp.append(float(entry[4]))
        ids.append(int(entry[0]))
    if not ids:
        raise ValueError(f"no simulation of split {an!r}" + (f" among {sorted(want)}" if want is not None else "") + f" under {data_dir}")
    sim = np.concatenate(sim)
    return dict(T=np.concatenate(T), u=np.concatenate(u), v=np.concatenate(v), sim=sim, prev=previous_snapshots(sim),
                raq=np.asarray(raq), fkt=np.asarray(fkt), fkp=np.asarray(fkp), xc=xc, yc=yc, sim_ids=ids)


def synthetic_series(N, H, W, seed=0):
    """Seeded stand-in for a series: the grid and temperature fields of rollout.synthetic_ensemble, velocities from a discrete
    stream function of a few modes that drifts from snapshot to snapshot, two simulations (N >= 2) with different parameters.
    Returns SeriesStore's arguments."""
    T, xc, yc = synthetic_ensemble(N, H, W, seed=seed)
    rng = np.random.RandomState(seed + 1)
    raq, fkt, fkp = np.array([1.5, 4.0]), np.array([1e6, 1e8]), np.array([10.0, 60.0])
    n0 = N - N // 2
    sim = np.concatenate([np.zeros(n0, np.int32), np.ones(N - n0, np.int32)])
    if N - n0 == 0:
        raq, fkt, fkp = raq[:1], fkt[:1], fkp[:1]
    scale = velocity_scaler(raq, fkt, fkp)
    y, x = np.meshgrid(np.linspace(0.0, 1.0, H + 2), np.linspace(0.0, 4.0, W + 2), indexing="ij")
    amp, ph = rng.uniform(0.5, 1.0, (2, 3)), rng.uniform(0.0, 2 * np.pi, (2, 3))
    u, v = np.zeros((N, H, W)), np.zeros((N, H, W))
    for n in range(N):
        s = sim[n]
        psi = sum(amp[s, m] * np.sin(np.pi * (m + 1) * y) * np.sin(0.5 * np.pi * (m + 1) * x + ph[s, m] + 0.05 * n) for m in range(3))
        u[n] = 0.5 * (psi[2:, 1:-1] - psi[:-2, 1:-1]) * scale[s]
        v[n] = -0.5 * (psi[1:-1, 2:] - psi[1:-1, :-2]) * scale[s]
    return dict(T=T[:, 0], u=u.astype(np.float32), v=v.astype(np.float32), sim=sim, prev=previous_snapshots(sim), raq=raq, fkt=fkt,
                fkp=fkp, xc=xc, yc=yc)


def load_rollout_truth(data_dir, an, sims=None, start=0, every=1, count=None):
    """One ensemble member per selected simulation of split `an` in the reference's layout: T0 = snapshot `start` of
    `e1_Tprev_data.pt`, truth = snapshots start + every, start + 2 every, ... (at most `count` of them) with the simulated times
    t = times[k] - times[start] from `times.pt` (snapshot i carries times[i], as the datasets pair them).  The mesh is loaded the
    way load_series loads it and mixed meshes are refused as there.  Series of different length are padded: n[m] holds the
    length, the padding times are +inf and the padding fields 0.  Returns the arguments of EnsembleRollout.reset -- T0
    [B,1,H,W], xc, yc, ycc, raq, fkt, fkp, nd, truth = dict(T [B,S,H,W], t [B,S], n [B]) -- plus sim_ids."""
    start, every = int(start), int(every)
    if start < 0 or every < 1 or (count is not None and int(count) < 1):
        raise ValueError("start must be non-negative, every and count at least 1")
    want = None if sims is None else {int(s) for s in sims}
    T0, Tt, tt, raq, fkt, fkp, ids = [], [], [], [], [], [], []
    xc = yc = None
    for entry, d in _selected_sims(str(data_dir), an):
        if want is not None and int(entry[0]) not in want:
            continue
        g = _Grid()
        g._load_grid(d)
        gx, gy = g.xc[0].numpy(), g.yc[0].numpy()
        if xc is None:
            xc, yc = gx, gy
        elif gx.shape != xc.shape or not (np.array_equal(gx, xc) and np.array_equal(gy, yc)):
            raise ValueError(f"an ensemble lives on one mesh: simulation {entry[0]} lies on another mesh than simulation {ids[0]}")
        H, W = xc.shape
        Ts = _load(d + "/e1_Tprev_data.pt").reshape(-1, H, W).float().numpy()
        times = torch.as_tensor(_load(d + "/times.pt")).to(torch.float64).reshape(-1).numpy()[:Ts.shape[0]]
        n_snap = min(Ts.shape[0], times.shape[0])
        if start >= n_snap:
            raise ValueError(f"{d}: snapshot {start} asked for, the series holds {n_snap}")
        ks = np.arange(start + every, n_snap, every)[:None if count is None else int(count)]
        T0.append(Ts[start]); Tt.append(Ts[ks]); tt.append(times[ks] - times[start])
        raq.append(float(entry[2])); fkt.append(float(entry[3])); fkp.append(float(entry[4]))
        ids.append(int(entry[0]))
    if not ids:
        raise ValueError(f"no simulation of split {an!r}" + (f" among {sorted(want)}" if want is not None else "") + f" under {data_dir}")
    B, S = len(ids), max(a.shape[0] for a in Tt)
    if S == 0:
        raise ValueError(f"no snapshot after snapshot {start} with every = {every}")
    T = np.zeros((B, S, H, W), dtype=np.float32)
    t = np.full((B, S), np.inf, dtype=np.float64)
    n = np.zeros(B, dtype=np.int32)
    for m in range(B):
        n[m] = Tt[m].shape[0]
        T[m, :n[m]], t[m, :n[m]] = Tt[m], tt[m]
    raq, fkt, fkp = np.asarray(raq), np.asarray(fkt), np.asarray(fkp)
    return dict(T0=np.stack(T0)[:, None].astype(np.float32), xc=xc, yc=yc, ycc=yc, raq=raq, fkt=fkt, fkp=fkp,
                nd=normalise_params(np.stack([raq, fkt, fkp], 1)), truth=dict(T=T, t=t, n=n), sim_ids=ids)


def synthetic_rollout_truth(B, S, H, W, seed=0):
    """Seeded stand-in for load_rollout_truth: initial and "simulated" fields from rollout.synthetic_ensemble, parameters that
    differ from member to member, and ascending times in pairs 1 % of a diffusive step apart (so two of them fall into one CFL
    step), the pairs three diffusive steps apart and shifted from member to member."""
    T0, xc, yc = synthetic_ensemble(B, H, W, seed=seed)
    T = synthetic_ensemble(B * S, H, W, seed=seed + 1)[0].reshape(B, S, H, W)
    dx, dy = 4.0 / (W - 2), 1.0 / (H - 2)
    step = 0.5 * dx * dx * dy * dy / (dx * dx + dy * dy)           # the diffusive limit of the explicit step: no CFL step is longer
    k = np.arange(S)
    t = (3.0 * step * (k // 2 + 1) + 0.01 * step * (k % 2))[None, :] * (1.0 + 0.125 * np.arange(B))[:, None]
    raq = np.array([1.5, 2.5, 4.0, 3.0])[np.arange(B) % 4]
    fkt = np.array([1e6, 1e7, 1e8, 1e7])[np.arange(B) % 4]
    fkp = np.array([10.0, 30.0, 60.0, 20.0])[np.arange(B) % 4]
    return dict(T0=T0, xc=xc, yc=yc, ycc=yc, raq=raq, fkt=fkt, fkp=fkp, nd=normalise_params(np.stack([raq, fkt, fkp], 1)),
                truth=dict(T=T, t=t.astype(np.float64), n=np.full(B, S, dtype=np.int32)), sim_ids=list(range(B)))


def summarise_rollout(score, level=0.9, sim_ids=None):
    """One dict per member from run()["score"] (tensors or arrays): the number of scored rows, the mean of mae over them, corr
    and prof_mae of the last scored row, the mean of |T_mean_pred - T_mean_true| (the three figures the reference's evaluation
    notebook puts into its titles) and the horizon: the first truth time whose corr is below `level`, inf if none is."""
    table = score["table"]
    table = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table, dtype=np.float64)
    col = {name: q for q, name in enumerate(ROLLOUT_SCORE_NAMES)}
    out = []
    for m in range(table.shape[0]):
        rows = table[m][~np.isnan(table[m][:, col["t"]])]
        d = dict(member=m if sim_ids is None else int(sim_ids[m]), scored=int(rows.shape[0]), level=float(level))
        if rows.shape[0]:
            low = rows[rows[:, col["corr"]] < level]
            d.update(mae=float(rows[:, col["mae"]].mean()), corr_last=float(rows[-1, col["corr"]]),
                     prof_mae_last=float(rows[-1, col["prof_mae"]]),
                     T_mean_mae=float(np.abs(rows[:, col["T_mean_pred"]] - rows[:, col["T_mean_true"]]).mean()),
                     t_last=float(rows[-1, col["t"]]), horizon=float(low[0, col["t"]]) if low.shape[0] else float("inf"))
        else:
            nan = float("nan")
            d.update(mae=nan, corr_last=nan, prof_mae_last=nan, T_mean_mae=nan, t_last=nan, horizon=float("inf"))
        out.append(d)
    return out


def write_rollout_scores(out_dir, score, summary, sim_ids=None):
    """rollout_scores.npz (table, names, prof, scored, skipped, next, sim) and rollout_summary.json (one line) under out_dir."""
    os.makedirs(out_dir, exist_ok=True)
    arr = lambda v: np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)  # noqa: E731
    npz, js = os.path.join(out_dir, "rollout_scores.npz"), os.path.join(out_dir, "rollout_summary.json")
    B = arr(score["table"]).shape[0]
    np.savez(npz, names=np.asarray(ROLLOUT_SCORE_NAMES), sim=np.asarray(list(range(B)) if sim_ids is None else sim_ids),
             **{k: arr(score[k]) for k in ("table", "prof", "scored", "skipped", "next")})
    with open(js, "w") as fh:
        fh.write(json.dumps(summary) + "\n")
    return npz, js


class SeriesScorer:
    """score(store, idx=None) -> dict(table [n_items,10] f64, names, profile [n_items,2,H] f64, idx [n_items], sim [n_items]).

    `stokes(inp [batch,7,H,W]) -> (u, v, p)` is a NewFluidNet (or a module around one) and belongs to this scorer: the
    captured step replays the engine's buffers of this (batch, H, W), and a forward of the same module at another shape
    re-plans them.  The step is captured once per (store shape, list length); a second store of the same shape is copied into
    the same device buffers and scored by the same graph."""

    def __init__(self, stokes, device, batch=32, precision=None, use_graph=True, scoring=True):
        from .pytorch_networks_convae import NewFluidNet
        mods = list(stokes.modules()) if isinstance(stokes, torch.nn.Module) else []
        if not any(isinstance(m, NewFluidNet) for m in mods):
            raise NotImplementedError("series scoring covers NewFluidNet (the deployed Stokes net); FluidNet, Unet and other "
                                      f"networks are not scored, got {type(stokes).__name__}")
        if isinstance(batch, bool) or int(batch) != batch or not 0 < int(batch) <= 65535:
            raise ValueError(f"batch must be an integer in [1, 65535], got {batch!r}")
        self.stokes, self.batch, self.use_graph = stokes, int(batch), bool(use_graph)
        self.device = device if isinstance(device, torch.device) else torch.device(device)
        self.scoring = bool(scoring)        # False: gather + forward alone (tools/bench_series_score.py times the difference)
        if precision is not None:
            stokes.set_precision(precision)
        self._g = None

    def _alloc(self, store, n_items):
        N, S, H, W = store.shape()
        dev, b = self.device, self.batch
        g = dict(key=(N, S, H, W, n_items), graph=None, out=None)
        for k in SeriesStore.TENSORS:
            g[k] = torch.empty_like(getattr(store, k), device=dev)
        g.update(idx=torch.zeros(n_items, dtype=torch.int32, device=dev), cursor=torch.zeros(1, dtype=torch.int32, device=dev),
                 inp=torch.empty((b, 7, H, W), dtype=torch.float32, device=dev),
                 rows=torch.zeros((b, len(SCORE_NAMES), H), dtype=torch.float64, device=dev),
                 table=torch.empty((n_items, len(SCORE_NAMES)), dtype=torch.float64, device=dev),
                 profile=torch.empty((n_items, 2, H), dtype=torch.float64, device=dev))
        self._g = g
        return g

    def _one_step(self):
        g = self._g
        N, S, H, W, n_items = g["key"]
        b, st = self.batch, L.stream()
        L.call("mc_series_build_input", L.ptr(g["T"]), H * W, L.ptr(g["sim"]), L.ptr(g["xc"]), L.ptr(g["yc"]), L.ptr(g["ycc"]),
               L.ptr(g["paras"]), L.ptr(g["nd"]), L.ptr(g["idx"]), L.ptr(g["cursor"]), n_items, N, S, b, H, W, L.ptr(g["inp"]), st)
        uu, vv, pp = self.stokes(g["inp"])
        uu, vv = uu.reshape(b, H, W), vv.reshape(b, H, W)
        # planes of the network's output tensor are read in place through their batch stride
        rows = lambda a: a.dtype == torch.float32 and a.stride(2) == 1 and a.stride(1) == W and a.stride(0) >= H * W  # noqa: E731
        if not (rows(uu) and rows(vv) and uu.stride(0) == vv.stride(0)):
            uu, vv = uu.float().contiguous(), vv.float().contiguous()
        g["out"] = (uu, vv, pp)
        if not self.scoring:
            return
        L.call("mc_series_score", L.ptr(uu), L.ptr(vv), int(uu.stride(0)), L.ptr(g["u"]), L.ptr(g["v"]), H * W, L.ptr(g["sim"]),
               L.ptr(g["prev"]), L.ptr(g["inv_scale"]), L.ptr(g["idx"]), L.ptr(g["cursor"]), n_items, N, S, b, H, W, L.ptr(g["rows"]), st)
        L.call("mc_series_score_finalize", L.ptr(g["rows"]), L.ptr(g["idx"]), L.ptr(g["cursor"]), n_items, N, b, H, W,
               L.ptr(g["table"]), L.ptr(g["profile"]), st)

    def _set_cursor(self, row):
        L.call("mc_series_set_cursor", L.ptr(self._g["cursor"]), int(row), self._g["key"][4], L.stream())

    def _start(self):
        """Results NaN, cursor at the head of the list."""
        self._g["table"].fill_(float("nan"))
        self._g["profile"].fill_(float("nan"))
        self._set_cursor(0)

    def _capture(self):
        g = self._g
        self._start()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._one_step()                                    # warm-up: allocates every buffer outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(self.device)
        self._start()                                           # the warm-up wrote rows and advanced the cursor: put them back
        g["graph"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g["graph"]):
            self._one_step()
        self._start()                                           # (a capture launches nothing; the cursor is set for the caller)

    @torch.no_grad()
    def score(self, store, idx=None):
        """Scores the snapshots idx (int indices into the store, any order, repeats allowed; None = all, in store order).
        Column names in `names`; the two baseline columns are NaN for a snapshot without a predecessor.  Nothing here waits
        for the device."""
        L.require_cuda(store.T, "the store")
        N = store.N
        ix = np.arange(N, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64).reshape(-1)
        if ix.size == 0 or ix.min() < 0 or ix.max() >= N:
            raise ValueError(f"idx must be a non-empty list of snapshot indices in [0, {N})")
        n_items = int(ix.size)
        with torch.cuda.device(self.device):
            g = self._g
            if g is None or g["key"] != store.shape() + (n_items,):
                g = self._alloc(store, n_items)
            # the captured step reads these buffers by address: refresh their CONTENTS, never the tensors
            for k in SeriesStore.TENSORS:
                g[k].copy_(getattr(store, k))
            g["idx"].copy_(torch.from_numpy(ix.astype(np.int32)))
            if self.use_graph and g["graph"] is None:
                self._capture()
            self._start()
            for _ in range((n_items + self.batch - 1) // self.batch):
                if self.use_graph:
                    g["graph"].replay()
                else:
                    self._one_step()
            idx_dev = g["idx"].clone()
            return dict(table=g["table"].clone(), names=SCORE_NAMES, profile=g["profile"].clone(), idx=idx_dev,
                        sim=g["sim"][idx_dev.long()])


# --------------------------------------------------------------------------------------------------
# CLI
# --------------------------------------------------------------------------------------------------
def build_arg_parser():
    p = argparse.ArgumentParser(description="Score a NewFluidNet checkpoint on the snapshots of a simulation series")
    p.add_argument("--weights", type=str, default=None, help="state_dict of the NewFluidNet (torch.save); seeded random weights if absent")
    p.add_argument("-l", "--levels", type=int, default=5)
    p.add_argument("-f", "--c_h", type=int, default=16)
    p.add_argument("-r", "--repeats", type=int, default=6)
    p.add_argument("-k", "--kernel", type=int, default=5)
    p.add_argument("-p", "--r_p", type=str, default="zeros")
    p.add_argument("-a", "--act_fn", type=str, default="gelu")
    p.add_argument("-lt", "--loss_type", type=str, default="mass")
    p.add_argument("-ab", "--a_bound", type=float, default=4.0, help="a_bound of the 'curl' head (the training run's -ab)")
    p.add_argument("-blurr", "--blurr", type=int, default=0, help="1: the net was trained with -blurr 1 (3 x 3 box mean of the "
                   "streamfunction inside the 'curl' head)")
    p.add_argument("--data_dir", type=str, default=None, help="directory with sims.pt and <an>/sim_<n>/")
    p.add_argument("--an", type=str, default="cv", help="split whose simulations are scored")
    p.add_argument("--sims", type=int, nargs="*", default=None, help="simulation numbers (default: all of the split)")
    p.add_argument("--every", type=int, default=1, help="score every k-th snapshot; the baseline is the preceding kept one")
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--precision", type=str, default=None, choices=["fp32", "bf16", "mixed"])
    p.add_argument("--graph", type=int, default=1)
    p.add_argument("--out", type=str, required=True)
    p.add_argument("--synthetic", type=int, nargs=3, metavar=("N", "H", "W"), default=None,
                   help="seeded synthetic grid, fields and velocities instead of --data_dir")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--rollout_steps", type=int, default=0,
                   help="N > 0: score the coupled rollout of N steps against the simulations instead -> rollout_scores.npz")
    p.add_argument("--start", type=int, default=0, help="rollout scoring: the snapshot the members start from")
    p.add_argument("--truth_every", type=int, default=1, help="rollout scoring: score against every k-th later snapshot")
    p.add_argument("--truth_count", type=int, default=None, help="rollout scoring: at most this many snapshots per member")
    p.add_argument("--t_end", type=float, default=None, help="rollout scoring: simulated time at which every member stops")
    p.add_argument("--level", type=float, default=0.9, help="rollout scoring: the horizon is the first time with corr below it")
    return p


def write_scores(out_dir, table, profile, idx, sim, sim_ids=None):
    """scores.npz (table, names, profile, idx, sim) and scores.csv (one line per item) under out_dir; returns their paths."""
    table, profile = np.asarray(table, dtype=np.float64), np.asarray(profile, dtype=np.float64)
    idx, sim = np.asarray(idx).reshape(-1), np.asarray(sim).reshape(-1)
    if table.shape != (idx.shape[0], len(SCORE_NAMES)) or sim.shape != idx.shape or profile.shape[:2] != (idx.shape[0], 2):
        raise ValueError("table [n,10], profile [n,2,H], idx [n] and sim [n] must describe the same items")
    os.makedirs(out_dir, exist_ok=True)
    npz, csv_path = os.path.join(out_dir, "scores.npz"), os.path.join(out_dir, "scores.csv")
    ids = np.asarray(sim if sim_ids is None else [sim_ids[s] for s in sim.tolist()])
    np.savez(npz, table=table, names=np.asarray(SCORE_NAMES), profile=profile, idx=idx, sim=ids)
    with open(csv_path, "w", newline="") as fh:
        wr = csv.writer(fh)
        wr.writerow(("item", "snapshot", "sim") + SCORE_NAMES)
        for j in range(idx.shape[0]):
            wr.writerow([j, int(idx[j]), int(ids[j])] + [repr(float(x)) for x in table[j]])
    return npz, csv_path


def summarise(table, sim, sim_ids=None):
    """One dict per simulation: the means of the ten columns over its items (the baseline columns over the items that have a
    baseline) and base/mae for u and v, the notebook's "baseline/prediction"."""
    table, sim = np.asarray(table, dtype=np.float64), np.asarray(sim).reshape(-1)
    out = []
    for s in sorted(set(sim.tolist())):
        rows = table[sim == s]
        mean = {}
        for q, name in enumerate(SCORE_NAMES):
            col = rows[:, q][~np.isnan(rows[:, q])]
            mean[name] = float(col.mean()) if col.size else float("nan")
        ratio = lambda a, b: a / b if b > 0 else float("nan")  # noqa: E731
        out.append(dict(sim=int(s if sim_ids is None else sim_ids[s]), snapshots=int(rows.shape[0]), **mean,
                        base_over_mae_u=ratio(mean["base_u"], mean["mae_u"]), base_over_mae_v=ratio(mean["base_v"], mean["mae_v"])))
    return out


def main(argv=None):
    a = build_arg_parser().parse_args(argv)
    if a.rollout_steps:
        return rollout_main(a)
    if a.synthetic:
        arrays = synthetic_series(*a.synthetic, seed=a.seed)
    elif a.data_dir:
        arrays = load_series(a.data_dir, a.an, sims=a.sims, every=a.every)
    else:
        raise SystemExit("give --data_dir DIR or --synthetic N H W")
    dev = torch.device(a.device)
    L.load()
    store = SeriesStore(**arrays, device=dev)
    scorer = SeriesScorer(build_stokes(a, dev), dev, batch=a.batch, precision=a.precision, use_graph=bool(a.graph))
    res = scorer.score(store)
    table, sim = res["table"].cpu().numpy(), res["sim"].cpu().numpy()
    write_scores(a.out, table, res["profile"].cpu().numpy(), res["idx"].cpu().numpy(), sim, store.sim_ids)
    lines = summarise(table, sim, store.sim_ids)
    for ln in lines:
        print(json.dumps(ln), flush=True)
    return lines


def rollout_main(a):
    """--rollout_steps N: truth from the files (or seeded), the ensemble rollout of the checkpoint, scores and summary."""
    if a.rollout_steps < 0:
        raise SystemExit("--rollout_steps must be positive")
    if a.synthetic:
        args = synthetic_rollout_truth(a.synthetic[0], a.truth_count or 4, a.synthetic[1], a.synthetic[2], seed=a.seed)
    elif a.data_dir:
        args = load_rollout_truth(a.data_dir, a.an, sims=a.sims, start=a.start, every=a.truth_every, count=a.truth_count)
    else:
        raise SystemExit("give --data_dir DIR or --synthetic B H W")
    ids = args.pop("sim_ids")
    dev = torch.device(a.device)
    L.load()
    ro = EnsembleRollout(build_stokes(a, dev), dev, precision=a.precision, use_graph=bool(a.graph),
                         score_capacity=int(args["truth"]["T"].shape[1]))
    ro.reset(**{k: (v if isinstance(v, dict) else torch.as_tensor(v)) for k, v in args.items()}, t_end=a.t_end)
    out = ro.run(a.rollout_steps)
    summary = dict(steps=a.rollout_steps, t=out["t"].cpu().tolist(), scored=out["score"]["scored"].cpu().tolist(),
                   skipped=out["score"]["skipped"].cpu().tolist(), members=summarise_rollout(out["score"], a.level, ids))
    write_rollout_scores(a.out, out["score"], summary, ids)
    print(json.dumps(summary), flush=True)
    return summary


if __name__ == "__main__":
    main()

"""Ensemble rollout: B simulations advance together on the device (DESIGN.md §8 "Ensemble rollout").

The deployed inference chain -- input builder -> NewFluidNet -> un-scale u, v -> explicit upwind advection-diffusion step --
for B members that differ in (RaQ, FKT, FKP) and in their temperature field.  Every member has its own CFL time step, its own
clock t[b] and its own stopping time t_end[b]; one step is captured as ONE HIP graph and replayed with no host
synchronisation inside the loop; six diagnostics per member and step are accumulated on the device.  `TS` + `ADNet`
(pytorch_networks_convae.py) stay the batch-1 restatement of the reference's wrapper; this module is beside them.

    python -m pbml_mantle_convection_amd.rollout --params params.csv --steps 100 --out DIR --synthetic 8 128 506 \
        -l 5 -f 16 -r 6 -k 5 -p zeros [--weights sd.pt] [--t_end X] [--snapshot_every K] [--precision bf16] \
        [--profiles 1 [--t_avg_start X]] [--save_every DT --save_capacity S] [--truth truth.npz [--score_capacity S]]
"""
import argparse
import json
import os

import numpy as np
import torch

from . import _lib as L
from .datasetio import normalise_parameters

HIST_NAMES = ("t", "dt", "T_mean", "v_rms", "Nu_bot", "Nu_top", "T_min", "T_max")
PROFILE_NAMES = ("T", "u2", "v2", "vT")           # rows of a depth profile: means over a row of T, (s u)^2, (s v)^2, (s v) T
SCORE_NAMES = ("t", "theta", "mae", "max_err", "corr", "prof_mae", "T_mean_pred", "T_mean_true")   # columns of a score row
HIST_CHUNK = 256          # rows of the device-side history buffer the captured step writes into


def broadcast_t_end(t_end, B):
    """None -> +inf (never stop), a number -> every member, [B] -> per member; f64 [B] on the host."""
    if t_end is None:
        return torch.full((B,), float("inf"), dtype=torch.float64)
    t = torch.as_tensor(t_end, dtype=torch.float64).detach().cpu().reshape(-1)
    if bool(torch.isnan(t).any()):
        raise ValueError("t_end must not be NaN")
    if t.numel() == 1:
        return t.expand(B).clone()
    if t.numel() != B:
        raise ValueError(f"t_end must be None, a number or hold one value per member ({B}), got {t.numel()} values")
    return t.clone()


def broadcast_member_value(value, B, name, default=0.0):
    """None -> `default` for every member, a number -> every member, [B] -> per member; f64 [B] on the host.  Negative and
    NaN values are refused (t_avg_start, save_every)."""
    if value is None:
        return torch.full((B,), float(default), dtype=torch.float64)
    t = torch.as_tensor(value, dtype=torch.float64).detach().cpu().reshape(-1)
    if bool(torch.isnan(t).any()) or bool((t < 0).any()):
        raise ValueError(f"{name} must be neither negative nor NaN")
    if t.numel() == 1:
        return t.expand(B).clone()
    if t.numel() != B:
        raise ValueError(f"{name} must be None, a number or hold one value per member ({B}), got {t.numel()} values")
    return t.clone()


def check_truth(truth, B, H, W, capacity):
    """truth = dict(T=[B,S,H,W], t=[B,S], n=[B] or None) with S <= capacity -> (T f32 [B,S,H,W], t f64 [B,S], n int32 [B]) on
    the host.  Within its first n[m] entries a member's times are finite, non-negative and strictly ascending."""
    if not isinstance(truth, dict) or "T" not in truth or "t" not in truth:
        raise ValueError("truth must be a dict with T [B,S,H,W], t [B,S] and optionally n [B]")
    T = torch.as_tensor(truth["T"]).detach().cpu()
    t = torch.as_tensor(truth["t"]).detach().cpu().to(torch.float64)
    if T.dim() != 4 or tuple(T.shape[:1] + T.shape[2:]) != (B, H, W):
        raise ValueError(f"truth['T'] must be [{B},S,{H},{W}], got {tuple(T.shape)}")
    S = int(T.shape[1])
    if S < 1 or S > capacity:
        raise ValueError(f"truth holds {S} snapshots per member, score_capacity is {capacity}")
    if tuple(t.shape) != (B, S):
        raise ValueError(f"truth['t'] must be [{B},{S}], got {tuple(t.shape)}")
    n = truth.get("n")
    n = torch.full((B,), S, dtype=torch.int64) if n is None else torch.as_tensor(n).detach().cpu().reshape(-1).to(torch.int64)
    if n.numel() != B or bool((n < 0).any()) or bool((n > S).any()):
        raise ValueError(f"truth['n'] must hold one count in [0, {S}] per member ({B})")
    for m in range(B):
        tm = t[m, :int(n[m])]
        if not bool(torch.isfinite(tm).all()) or bool((tm < 0).any()) or bool((tm[1:] <= tm[:-1]).any()):
            raise ValueError(f"truth['t'][{m}] must be finite, non-negative and strictly ascending within its {int(n[m])} entries")
    return T.to(torch.float32), t, n.to(torch.int32)


def parse_params_csv(path):
    """One row `raq,fkt,fkp` per member (blank lines, `#` comments and one header line are skipped) -> float64 [B, 3]."""
    rows = []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            s = line.split("#", 1)[0].strip()
            if not s:
                continue
            cells = [c.strip() for c in s.split(",")]
            try:
                vals = [float(c) for c in cells]
            except ValueError:
                if not rows and len(cells) == 3:
                    continue                                    # header
                raise ValueError(f"{path}:{ln}: expected three numbers raq,fkt,fkp, got {line.strip()!r}")
            if len(vals) != 3:
                raise ValueError(f"{path}:{ln}: expected three numbers raq,fkt,fkp, got {len(vals)}")
            if vals[1] <= 0 or vals[2] <= 0:
                raise ValueError(f"{path}:{ln}: fkt and fkp must be positive")
            rows.append(vals)
    if not rows:
        raise ValueError(f"{path}: no parameter rows")
    return np.asarray(rows, dtype=np.float64)


def normalise_params(paras):
    """[B, 3] (RaQ, FKT, FKP) -> [B, 3] network inputs with the dataset's ranges (datasetio.normalise_parameters)."""
    p = np.asarray(paras, dtype=np.float64).reshape(-1, 3)
    return np.stack(normalise_parameters(p[:, 0], p[:, 1], p[:, 2]), axis=1)


def synthetic_ensemble(B, H, W, seed=0):
    """Cell-centred grid with the wall coordinates in the first / last row and column, and B conductive profiles with a few
    plumes each (row 0 = bottom, T = 1): what the CLI runs on when the simulation files are absent.
    Returns float32 (T0 [B,1,H,W], xc [H,W], yc [H,W])."""
    xs = np.concatenate(([0.0], (np.arange(W - 2) + 0.5) * 4.0 / (W - 2), [4.0]))
    ys = np.concatenate(([0.0], (np.arange(H - 2) + 0.5) * 1.0 / (H - 2), [1.0]))
    xc = np.broadcast_to(xs[None, :], (H, W)).copy()
    yc = np.broadcast_to(ys[:, None], (H, W)).copy()
    rng = np.random.RandomState(seed)
    T0 = np.zeros((B, 1, H, W))
    for b in range(B):
        T = 1.0 - yc
        for _ in range(4):
            a, s = rng.uniform(0.05, 0.3), rng.uniform(0.03, 0.15)
            cx, cy = rng.uniform(0, 4), rng.uniform(0, 1)
            T = T + a * np.exp(-((xc - cx) ** 2 + (yc - cy) ** 2) / (2 * s * s))
        T = np.clip(T, 0.0, 1.35)
        T[0, :], T[-1, :] = 1.0, 0.0
        T0[b, 0] = T
    return T0.astype(np.float32), xc.astype(np.float32), yc.astype(np.float32)


class EnsembleRollout:
    """reset(...) loads B members, run(n) advances every active member n steps and returns the fields, clocks and history.

    State (plain tensors on `device`): T [B,1,H,W] f32, t [B] f64, t_end [B] f64 (+inf = never stop), steps [B] int32.  A
    member is active iff t < t_end; a step that would cross t_end is shortened and lands ON it; an inactive member is frozen
    (its T is copied, its dt is 0).

    `stokes(inp [B,7,H,W]) -> (u, v, p)` is a NewFluidNet (or a module around one); it belongs to this rollout: the captured
    step replays the engine's buffers of this (B, H, W), and a forward of the same module at another shape re-plans them.

    `profiles=True` adds mc_ensemble_profiles to the step: the horizontally averaged T, (s u)^2, (s v)^2 and (s v) T of the
    state every step starts from, and their time-weighted sums from t_avg_start[b] on.  `save_capacity=S > 0` adds
    mc_ensemble_snapshot: up to S fields per member and run, saved when the member's own clock passes its next saving time
    (save_every[b] apart).  With both off the step issues the same launches as before and nothing else changes.

    `score_capacity=S > 0` adds mc_score_rollout between the step and its finalize: each member carries up to S later
    snapshots of its simulation with their simulated times (reset(..., truth=...)), and the step in which the member's own
    clock passes one of those times scores the member's temperature, interpolated linearly in time between the state before
    and after the step, against that snapshot (SCORE_NAMES).  With score_capacity = 0 nothing is allocated or launched."""

    def __init__(self, stokes, device, CN_max=0.1, precision=None, use_graph=True, profiles=False, save_capacity=0,
                 score_capacity=0):
        self.stokes, self.CN_max, self.use_graph = stokes, float(CN_max), bool(use_graph)
        self.device = device if isinstance(device, torch.device) else torch.device(device)
        if isinstance(save_capacity, bool) or int(save_capacity) != save_capacity or int(save_capacity) < 0:
            raise ValueError(f"save_capacity must be a non-negative integer, got {save_capacity!r}")
        if isinstance(score_capacity, bool) or int(score_capacity) != score_capacity or int(score_capacity) < 0:
            raise ValueError(f"score_capacity must be a non-negative integer, got {score_capacity!r}")
        self.profiles, self.save_capacity, self.score_capacity = bool(profiles), int(save_capacity), int(score_capacity)
        if precision is not None:
            stokes.set_precision(precision)
        self._s = None          # member state
        self._x = None          # statistics of the members (profiles / save_capacity): the captured step reads them by address
        self._sc = None         # truth and scores of the members (score_capacity): read and written by address as well
        self._g = None          # grid, parameters, work buffers and the captured step of one (B, H, W)

    # ---- member state ---------------------------------------------------------------------------------------------
    def _alloc_state(self, B, H, W):
        if self._s is None or tuple(self._s["T"].shape) != (B, 1, H, W):
            dev = self.device
            self._s = dict(T=torch.zeros((B, 1, H, W), dtype=torch.float32, device=dev),
                           t=torch.zeros(B, dtype=torch.float64, device=dev),
                           t_end=torch.full((B,), float("inf"), dtype=torch.float64, device=dev),
                           steps=torch.zeros(B, dtype=torch.int32, device=dev))
            self._g = None      # the captured step reads the state by address
            if self.profiles or self.save_capacity:
                f64, i32, S = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev), self.save_capacity
                self._x = dict(t_avg_start=torch.zeros(B, **f64), acc=torch.zeros((B, 4, H), **f64), last=torch.zeros((B, 4, H), **f64),
                               weight=torch.zeros(B, **f64), count=torch.zeros(B, **i32), save_every=torch.zeros(B, **f64),
                               next_save=torch.zeros(B, **f64), saved=torch.zeros(B, **i32), missed=torch.zeros(B, **i32),
                               slot=torch.full((B,), -1, **i32))
                if S:
                    self._x.update(snaps=torch.zeros((B, S, H, W), dtype=torch.float32, device=dev),
                                   snap_t=torch.full((B, S), float("nan"), **f64))
            if self.score_capacity:
                f64, i32, S = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev), self.score_capacity
                self._sc = dict(truth=torch.zeros((B, S, H, W), dtype=torch.float32, device=dev),
                                truth_t=torch.full((B, S), float("inf"), **f64), n=torch.zeros(B, **i32), next=torch.zeros(B, **i32),
                                scored=torch.zeros(B, **i32), skipped=torch.zeros(B, **i32),
                                table=torch.full((B, S, len(SCORE_NAMES)), float("nan"), **f64),
                                prof=torch.full((B, S, 2, H), float("nan"), **f64))
        return self._s

    STATS_KEYS = ("acc", "weight", "count", "next_save")
    SCORE_KEYS = ("next", "scored", "skipped", "table", "prof")

    def state(self):
        """Copies of T, t, t_end, steps: enough to stop a study and continue it (load_state) on the same grid and parameters.
        With profiles or timed saves on, also "stats": the time sums acc [B,4,H], their weight [B] and count [B], next_save [B];
        with scoring on, also "score": next, scored, skipped [B], table [B,S,8], prof [B,S,2,H] (the truth itself comes from
        reset)."""
        if self._s is None:
            raise RuntimeError("no state: call reset() or load_state() first")
        st = {k: v.clone() for k, v in self._s.items()}
        if self._x is not None:
            st["stats"] = {k: self._x[k].clone() for k in self.STATS_KEYS}
        if self._sc is not None:
            st["score"] = {k: self._sc[k].clone() for k in self.SCORE_KEYS}
        return st

    def load_state(self, state):
        T = torch.as_tensor(state["T"])
        if T.dim() == 3:
            T = T.unsqueeze(1)
        if T.dim() != 4 or T.shape[1] != 1:
            raise ValueError(f"state['T'] must be [B,1,H,W], got {tuple(T.shape)}")
        B, _, H, W = T.shape
        for k in ("t", "t_end", "steps"):
            if torch.as_tensor(state[k]).numel() != B:
                raise ValueError(f"state[{k!r}] must hold one value per member ({B})")
        s = self._alloc_state(B, H, W)
        s["T"].copy_(T.to(torch.float32))
        s["t"].copy_(torch.as_tensor(state["t"]).reshape(B).to(torch.float64))
        s["t_end"].copy_(torch.as_tensor(state["t_end"]).reshape(B).to(torch.float64))
        s["steps"].copy_(torch.as_tensor(state["steps"]).reshape(B).to(torch.int32))
        stats = state.get("stats")
        if stats is not None:
            if self._x is None:
                raise ValueError("state['stats'] needs a rollout built with profiles=True or save_capacity > 0")
            for k in self.STATS_KEYS:
                v = torch.as_tensor(stats[k])
                if v.numel() != self._x[k].numel():
                    raise ValueError(f"state['stats'][{k!r}] must hold {tuple(self._x[k].shape)}")
                self._x[k].copy_(v.reshape(self._x[k].shape).to(self._x[k].dtype))
        score = state.get("score")
        if score is not None:
            if self._sc is None:
                raise ValueError("state['score'] needs a rollout built with score_capacity > 0")
            for k in self.SCORE_KEYS:
                v = torch.as_tensor(score[k])
                if v.numel() != self._sc[k].numel():
                    raise ValueError(f"state['score'][{k!r}] must hold {tuple(self._sc[k].shape)}")
            for k in self.SCORE_KEYS:
                self._sc[k].copy_(torch.as_tensor(score[k]).reshape(self._sc[k].shape).to(self._sc[k].dtype))
        return self

    # ---- grid and parameters --------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset(self, T0, xc, yc, ycc, raq, fkt, fkp, nd, t_end=None, t_avg_start=None, save_every=None, truth=None):
        """T0 [B,1,H,W]; xc, yc, ycc [H,W] (ycc: the depth coordinate of the viscosity law, TS's `ycc`); raq, fkt, fkp [B];
        nd [B,3] their normalised values (normalise_params); t_end None | number | [B].  Clocks and step counts restart at 0.
        t_avg_start None (= 0) | number | [B]: the time from which the profiles are averaged (needs profiles=True);
        save_every None (= never) | number | [B]: the simulated time between two timed saves (needs save_capacity > 0).  The
        time sums and the save counters restart at 0 and the first saving time is 0, so a saving member's first step is saved.
        truth None | dict(T=[B,S,H,W], t=[B,S], n=[B] or None), S <= score_capacity: the later snapshots of each member's
        simulation and their simulated times (needs score_capacity > 0); the scores restart: rows NaN, counters 0.  With
        scoring on and no truth nothing is ever scored."""
        T0 = torch.as_tensor(T0)
        if T0.dim() != 4 or T0.shape[1] != 1:
            raise ValueError(f"T0 must be [B,1,H,W], got {tuple(T0.shape)}")
        B, _, H, W = T0.shape
        if H < 5 or W < 5:
            raise ValueError("the grid must be at least 5 x 5")
        if t_avg_start is not None and not self.profiles:
            raise ValueError("t_avg_start needs EnsembleRollout(..., profiles=True)")
        if save_every is not None and not self.save_capacity:
            raise ValueError("save_every needs EnsembleRollout(..., save_capacity=S) with S > 0")
        if truth is not None:
            if not self.score_capacity:
                raise ValueError("truth needs EnsembleRollout(..., score_capacity=S) with S > 0")
            truth = check_truth(truth, B, H, W, self.score_capacity)
        tas = broadcast_member_value(t_avg_start, B, "t_avg_start")
        sev = broadcast_member_value(save_every, B, "save_every")           # 0 = never
        dev = self.device
        f = dict(dtype=torch.float32, device=dev)
        te = broadcast_t_end(t_end, B)
        vec = lambda a: torch.as_tensor(a, dtype=torch.float32).reshape(-1)  # noqa: E731
        paras = torch.stack([vec(raq), vec(fkt), vec(fkp)], 1)
        ndt = torch.as_tensor(nd, dtype=torch.float32).reshape(-1, 3)
        if paras.shape[0] != B or ndt.shape[0] != B:
            raise ValueError(f"raq, fkt, fkp and nd must hold one row per member ({B})")
        plane = lambda a: torch.as_tensor(a).to(**f).reshape(-1, H, W)[0].contiguous()  # noqa: E731
        s = self._alloc_state(B, H, W)
        s["T"].copy_(T0.to(**f))
        s["t"].zero_()
        s["steps"].zero_()
        s["t_end"].copy_(te)
        x = self._x
        if x is not None:
            x["t_avg_start"].copy_(tas); x["save_every"].copy_(sev)
            for k in ("acc", "weight", "count", "next_save", "saved", "missed"):
                x[k].zero_()
        sc = self._sc
        if sc is not None:
            sc["truth"].zero_(); sc["truth_t"].fill_(float("inf")); sc["n"].zero_()
            if truth is not None:
                S = truth[0].shape[1]
                sc["truth"][:, :S].copy_(truth[0]); sc["truth_t"][:, :S].copy_(truth[1]); sc["n"].copy_(truth[2])
            for k in ("next", "scored", "skipped"):
                sc[k].zero_()
            sc["table"].fill_(float("nan")); sc["prof"].fill_(float("nan"))
        g = self._g
        if g is None:
            nblk = L.call("mc_rollout_blocks", H, W)
            g = self._g = dict(shape=(B, H, W), graph=None, out=None,
                               xc=torch.empty((H, W), **f), yc=torch.empty((H, W), **f), ycc=torch.empty((H, W), **f),
                               paras=torch.empty((B, 3), **f), nd=torch.empty((B, 3), **f), raq=torch.empty(B, **f),
                               scaler=torch.empty(B, **f), inp=torch.empty((B, 7, H, W), **f), Tn=torch.empty((B, H, W), **f),
                               dx_min=torch.empty(1, **f), ws=torch.zeros(B, dtype=torch.int32, device=dev),
                               dt=torch.zeros(B, dtype=torch.float64, device=dev),
                               flags=torch.zeros(B, dtype=torch.int32, device=dev),
                               part=torch.zeros(B * nblk * 8, dtype=torch.float64, device=dev),
                               cursor=torch.zeros(1, dtype=torch.int32, device=dev),
                               hist=torch.zeros((HIST_CHUNK, B, 8), dtype=torch.float64, device=dev))
        # the captured step reads these buffers by address: refresh their CONTENTS, never the tensors
        paras = paras.to(**f)
        g["xc"].copy_(plane(xc)); g["yc"].copy_(plane(yc)); g["ycc"].copy_(plane(ycc))
        g["paras"].copy_(paras); g["nd"].copy_(ndt.to(**f)); g["raq"].copy_(paras[:, 0])
        g["scaler"].copy_(torch.exp(paras[:, 0] / 10 * 1.80167667 + torch.log(paras[:, 1]) * 0.4330392
                                    + torch.log(paras[:, 2]) * -0.46052953) * 5)              # TS's un-scaling factor
        L.call("mc_rollout_dx_min", L.ptr(g["xc"]), H, W, L.ptr(g["dx_min"]), L.stream())
        return self

    # ---- one step ---------------------------------------------------------------------------------------------------
    def _one_step(self):
        s, g = self._s, self._g
        B, H, W = g["shape"]
        st = L.stream()
        L.call("mc_ts_build_input", L.ptr(s["T"]), L.ptr(g["xc"]), L.ptr(g["yc"]), L.ptr(g["ycc"]), L.ptr(g["paras"]),
               L.ptr(g["nd"]), B, H, W, L.ptr(g["inp"]), st)
        uu, vv, pp = self.stokes(g["inp"])
        uu, vv = uu.reshape(B, H, W), vv.reshape(B, H, W)
        # planes of the network's output tensor are read in place through their batch stride
        rows = lambda a: a.dtype == torch.float32 and a.stride(2) == 1 and a.stride(1) == W and a.stride(0) >= H * W  # noqa: E731
        if not (rows(uu) and rows(vv) and uu.stride(0) == vv.stride(0)):
            uu, vv = uu.float().contiguous(), vv.float().contiguous()
        uvs = int(uu.stride(0))
        L.call("mc_rollout_dt", L.ptr(uu), L.ptr(vv), uvs, L.ptr(g["scaler"]), L.ptr(g["dx_min"]), L.ptr(s["t"]),
               L.ptr(s["t_end"]), B, H, W, self.CN_max, L.ptr(g["ws"]), L.ptr(g["dt"]), L.ptr(g["flags"]), st)
        x = self._x
        if self.profiles:                                       # the state this step starts from, before t and T advance
            L.call("mc_ensemble_profiles", L.ptr(uu), L.ptr(vv), uvs, L.ptr(g["scaler"]), L.ptr(s["T"]), L.ptr(g["dt"]),
                   L.ptr(g["flags"]), L.ptr(s["t"]), L.ptr(x["t_avg_start"]), B, H, W, L.ptr(x["last"]), L.ptr(x["acc"]),
                   L.ptr(x["weight"]), L.ptr(x["count"]), st)
        L.call("mc_rollout_step", L.ptr(uu), L.ptr(vv), uvs, L.ptr(g["scaler"]), L.ptr(s["T"]), L.ptr(g["raq"]),
               L.ptr(g["xc"]), L.ptr(g["yc"]), L.ptr(g["dt"]), L.ptr(g["flags"]), B, H, W, L.ptr(g["Tn"]), L.ptr(g["part"]), st)
        if self.score_capacity:                                 # T_next is written, t is still the old clock
            sc = self._sc
            L.call("mc_score_rollout", L.ptr(s["T"]), L.ptr(g["Tn"]), L.ptr(s["t"]), L.ptr(g["dt"]), L.ptr(g["flags"]), L.ptr(s["t_end"]),
                   L.ptr(sc["truth"]), L.ptr(sc["truth_t"]), L.ptr(sc["n"]), self.score_capacity, B, H, W, L.ptr(sc["next"]),
                   L.ptr(sc["scored"]), L.ptr(sc["skipped"]), L.ptr(sc["table"]), L.ptr(sc["prof"]), st)
        L.call("mc_rollout_finalize", L.ptr(g["part"]), L.ptr(g["dt"]), L.ptr(g["flags"]), L.ptr(s["t_end"]), L.ptr(s["t"]),
               L.ptr(s["steps"]), L.ptr(g["cursor"]), L.ptr(g["hist"]), HIST_CHUNK, B, H, W, st)
        if self.save_capacity:                                  # the new clock and the field just written
            L.call("mc_ensemble_snapshot", L.ptr(g["Tn"]), L.ptr(s["t"]), L.ptr(g["flags"]), L.ptr(x["save_every"]),
                   L.ptr(x["next_save"]), L.ptr(x["saved"]), L.ptr(x["missed"]), L.ptr(x["slot"]), self.save_capacity, B, H, W,
                   L.ptr(x["snaps"]), L.ptr(x["snap_t"]), st)
        s["T"].view(B, H, W).copy_(g["Tn"])
        g["out"] = (uu, vv, pp)

    def _set_cursor(self, row):
        L.call("mc_rollout_set_cursor", L.ptr(self._g["cursor"]), int(row), HIST_CHUNK, L.stream())

    def _capture(self):
        s, g = self._s, self._g
        keep = {k: s[k].clone() for k in ("T", "t", "steps")}
        xkeep = {k: v.clone() for k, v in self._x.items()} if self._x is not None else {}
        sckeep = {k: self._sc[k].clone() for k in self.SCORE_KEYS} if self._sc is not None else {}
        self._set_cursor(0)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._one_step()                                    # warm-up: allocates every buffer outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(self.device)
        for k, v in keep.items():                               # the warm-up advanced the members: put them back
            s[k].copy_(v)
        for k, v in xkeep.items():                              # ... and their statistics
            self._x[k].copy_(v)
        for k, v in sckeep.items():                             # ... and their scores
            self._sc[k].copy_(v)
        g["graph"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g["graph"]):
            self._one_step()

    @torch.no_grad()
    def run(self, n_steps, snapshot_every=0):
        """Advance n_steps (members past their t_end stay frozen); continues where the last run ended.  Returns a dict: T
        [B,1,H,W], t [B] f64, steps [B] int32, hist [n_steps,B,8] f64 with the columns `names`, snapshots [S,B,H,W] (the
        states after every snapshot_every-th step of this run) or None, and u, v, p of the last step, un-scaled as TS
        returns them; `profiles` (None, or names, acc [B,4,H], weight [B], count [B], mean = acc / weight where weight > 0
        else 0, last [B,4,H]: the profile of the state the last step started from) and `timed` (None, or T [B,S,H,W],
        t [B,S], count [B], missed [B]: the fields saved during THIS run at each member's saving times, slots from count[b]
        on are stale and their t is NaN; the next saving time carries over to the next run) and `score` (None, or names =
        SCORE_NAMES, table [B,S,8], prof [B,S,2,H] = the row means of prediction and truth, scored [B], skipped [B], next [B]:
        cumulative since reset(), rows not scored yet are NaN).  Nothing here waits for the device."""
        if self._g is None or self._s is None:
            raise RuntimeError("call reset() first (load_state() alone carries no grid and no parameters)")
        n_steps, every = int(n_steps), int(snapshot_every)
        if n_steps <= 0 or every < 0:
            raise ValueError("n_steps must be positive and snapshot_every non-negative")
        L.require_cuda(self._s["T"], "the ensemble state")
        s, g = self._s, self._g
        B, H, W = g["shape"]
        dev = self.device
        with torch.cuda.device(dev):
            if self.use_graph and g["graph"] is None:
                self._capture()
            x = self._x
            if self.save_capacity:                              # the timed snapshots returned belong to this run
                x["saved"].zero_(); x["missed"].zero_(); x["snap_t"].fill_(float("nan"))
            hist = torch.empty((n_steps, B, 8), dtype=torch.float64, device=dev)
            snaps = torch.empty((n_steps // every, B, H, W), dtype=torch.float32, device=dev) if every else None
            done = 0
            while done < n_steps:
                chunk = min(HIST_CHUNK, n_steps - done)
                self._set_cursor(0)
                for i in range(chunk):
                    if self.use_graph:
                        g["graph"].replay()
                    else:
                        self._one_step()
                    k = done + i + 1
                    if every and k % every == 0:
                        snaps[k // every - 1].copy_(s["T"].view(B, H, W))
                hist[done:done + chunk].copy_(g["hist"][:chunk])
                done += chunk
            u, v, p = g["out"]
            sv = g["scaler"].view(B, 1, 1, 1)
            prof = timed = score = None
            if self.profiles:
                acc, wt = x["acc"].clone(), x["weight"].clone()
                mean = torch.where(wt.view(B, 1, 1) > 0, acc / wt.view(B, 1, 1), torch.zeros_like(acc))
                prof = dict(names=PROFILE_NAMES, acc=acc, weight=wt, count=x["count"].clone(), mean=mean, last=x["last"].clone())
            if self.save_capacity:
                timed = dict(T=x["snaps"].clone(), t=x["snap_t"].clone(), count=x["saved"].clone(), missed=x["missed"].clone())
            if self.score_capacity:
                sc = self._sc
                score = dict(names=SCORE_NAMES, table=sc["table"].clone(), prof=sc["prof"].clone(), scored=sc["scored"].clone(),
                             skipped=sc["skipped"].clone(), next=sc["next"].clone())
            return dict(T=s["T"].clone(), t=s["t"].clone(), steps=s["steps"].clone(), hist=hist, names=HIST_NAMES,
                        snapshots=snaps, u=u.unsqueeze(1) * sv, v=v.unsqueeze(1) * sv,
                        p=p.reshape(B, 1, H, W) if p is not None else None, profiles=prof, timed=timed, score=score)


# --------------------------------------------------------------------------------------------------
# CLI
# --------------------------------------------------------------------------------------------------
def build_arg_parser():
    p = argparse.ArgumentParser(description="Ensemble rollout of the deployed surrogate (NewFluidNet + advection-diffusion step)")
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
    p.add_argument("--params", type=str, required=True, help="CSV: one row raq,fkt,fkp per member")
    p.add_argument("--steps", type=int, required=True)
    p.add_argument("--t_end", type=float, default=None)
    p.add_argument("--snapshot_every", type=int, default=0)
    p.add_argument("--profiles", type=int, default=0, help="1: depth profiles and their time averages -> profiles.npz")
    p.add_argument("--t_avg_start", type=float, default=None, help="simulated time from which the profiles are averaged")
    p.add_argument("--save_every", type=float, default=None, help="simulated time between two saved fields of a member")
    p.add_argument("--save_capacity", type=int, default=0, help="saved fields per member -> timed_snapshots.npz")
    p.add_argument("--truth", type=str, default=None,
                   help=".npz with T [B,S,H,W], t [B,S] and optionally n [B]: snapshots the members are scored against -> scores.npz")
    p.add_argument("--score_capacity", type=int, default=0, help="scored snapshots per member (default: what --truth holds)")
    p.add_argument("--out", type=str, required=True)
    p.add_argument("--synthetic", type=int, nargs=3, metavar=("B", "H", "W"), default=None,
                   help="seeded synthetic grid and initial fields instead of --init")
    p.add_argument("--init", type=str, default=None, help=".npz with T0 [B,H,W], xc, yc [H,W] and optionally ycc")
    p.add_argument("--precision", type=str, default=None, choices=["fp32", "bf16", "mixed"])
    p.add_argument("--CN_max", type=float, default=0.1)
    p.add_argument("--graph", type=int, default=1)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=str, default="cuda:0")
    return p


def build_stokes(a, dev):
    """The NewFluidNet of the command line (7 input channels, u / v / p outputs), weights from --weights or seeded.  The output
    channels are the training command line's (`multigpu.channels_for`: 3, or 2 with `-lt curl`, whose streamfunction stands for
    u and v), so that a checkpoint of `-lt curl [-blurr 1] -pp 1` loads; `-ab` is that run's a_bound."""
    from .multigpu import channels_for
    from .pytorch_networks_convae import NewFluidNet
    torch.manual_seed(a.seed)
    m = NewFluidNet(a.levels, 7, a.c_h, channels_for("newfluidnet", a.loss_type, True)[1], dev, a.act_fn, a.r_p, a.loss_type,
                    use_symm=True, a_bound=getattr(a, "a_bound", 4.0), repeats=a.repeats, f=a.kernel, p_pred=True,
                    blurr=getattr(a, "blurr", 0) == 1)
    if a.weights:
        m.load_state_dict(torch.load(a.weights, map_location="cpu"))
    return m.to(dev)


def main(argv=None):
    a = build_arg_parser().parse_args(argv)
    paras = parse_params_csv(a.params)
    B = paras.shape[0]
    if a.synthetic:
        if a.synthetic[0] != B:
            raise SystemExit(f"--synthetic asks for {a.synthetic[0]} members, {a.params} holds {B}")
        T0, xc, yc = synthetic_ensemble(*a.synthetic, seed=a.seed)
        ycc = yc
    elif a.init:
        z = np.load(a.init)
        xc, yc = z["xc"], z["yc"]
        ycc = z["ycc"] if "ycc" in z.files else yc
        T0 = np.asarray(z["T0"], dtype=np.float32).reshape(-1, 1, *xc.shape[-2:])
        if T0.shape[0] == 1 and B > 1:
            T0 = np.repeat(T0, B, axis=0)
        if T0.shape[0] != B:
            raise SystemExit(f"{a.init} holds {T0.shape[0]} initial fields, {a.params} holds {B} members")
    else:
        raise SystemExit("give --synthetic B H W or --init FILE")
    truth = None
    if a.truth:
        z = np.load(a.truth)
        truth = dict(T=np.asarray(z["T"], dtype=np.float32), t=np.asarray(z["t"], dtype=np.float64),
                     n=z["n"] if "n" in z.files else None)
    elif a.score_capacity:
        raise SystemExit("--score_capacity needs --truth FILE.npz")
    dev = torch.device(a.device)
    L.load()
    ro = EnsembleRollout(build_stokes(a, dev), dev, CN_max=a.CN_max, precision=a.precision, use_graph=bool(a.graph),
                         profiles=bool(a.profiles), save_capacity=a.save_capacity,
                         score_capacity=a.score_capacity or (truth["T"].shape[1] if truth is not None else 0))
    ro.reset(torch.from_numpy(T0), torch.from_numpy(xc), torch.from_numpy(yc), torch.from_numpy(ycc), paras[:, 0], paras[:, 1],
             paras[:, 2], normalise_params(paras), t_end=a.t_end, t_avg_start=a.t_avg_start, save_every=a.save_every, truth=truth)
    out = ro.run(a.steps, snapshot_every=a.snapshot_every)
    os.makedirs(a.out, exist_ok=True)
    hist = out["hist"].cpu().numpy()
    final_T = out["T"].cpu().numpy()
    snaps = out["snapshots"].cpu().numpy() if out["snapshots"] is not None else np.zeros((0, B) + final_T.shape[-2:], np.float32)
    np.save(os.path.join(a.out, "hist.npy"), hist)
    np.save(os.path.join(a.out, "final_T.npy"), final_T)
    np.save(os.path.join(a.out, "snapshots.npy"), snaps)
    summary = dict(members=B, grid=list(final_T.shape[-2:]), steps=a.steps, names=list(HIST_NAMES),
                   weights=a.weights or f"random (seed {a.seed})", t=out["t"].cpu().tolist(),
                   member_steps=out["steps"].cpu().tolist(), T_mean=hist[-1, :, 2].tolist(), v_rms=hist[-1, :, 3].tolist(),
                   snapshots=int(snaps.shape[0]), finite=bool(np.isfinite(final_T).all()))
    if out["profiles"] is not None:
        pr = {k: (list(v) if k == "names" else v.cpu().numpy()) for k, v in out["profiles"].items()}
        np.savez(os.path.join(a.out, "profiles.npz"), **pr)
        summary["profiles"] = dict(names=pr["names"], weight=pr["weight"].tolist(), count=pr["count"].tolist())
    if out["timed"] is not None:
        tm = {k: v.cpu().numpy() for k, v in out["timed"].items()}
        np.savez(os.path.join(a.out, "timed_snapshots.npz"), **tm)
        summary["timed"] = dict(count=tm["count"].tolist(), missed=tm["missed"].tolist())
    if out["score"] is not None:
        from .evaluate import summarise_rollout
        sc = {k: (list(v) if k == "names" else v.cpu().numpy()) for k, v in out["score"].items()}
        np.savez(os.path.join(a.out, "scores.npz"), **sc)
        summary["score"] = summarise_rollout(sc)
    line = json.dumps(summary)
    with open(os.path.join(a.out, "summary.json"), "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)
    return summary


if __name__ == "__main__":
    main()

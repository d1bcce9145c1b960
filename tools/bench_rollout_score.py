#!/usr/bin/env python3
"""Cost of rollout scoring: milliseconds per captured step of the ensemble rollout with

    off        score_capacity = 0: the launches of the rollout without the feature
    idle       scoring on, no truth time due in the timed steps (the common step: one near-empty graph node)
    staggered  scoring on, one truth time due per member about every tenth step, staggered across the members
    burst      scoring on, every member due in the same step, about every tenth step

and what a user does without the feature for the same scores (without interpolation): `run(1)` per step, a host read of the
clocks, and torch expressions per due snapshot ("host_loop", on the staggered truth).

The method of tools/bench_ensemble_stats.py: the deployed configuration (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros,
128 x 506, bf16, seeded weights and fields), `EnsembleRollout(use_graph=True)` at B = 32 and 8, in one process, alternating
--repeats times so that all variants see the same box in the same state.  A timed window is --steps rollout steps between two
device events, ended by a synchronise; every window starts from reset(), outside the timed region, so that every window of a
variant does the same work.  The truth times are multiples of each member's own mean time step, measured beforehand.  A due
snapshot reads three planes twice: 6 x 128 x 506 x 4 B = 1.55 MB per member.  Prints one JSON line and writes it to --out.
--only VARIANT --batches B runs one variant alone (for a kernel trace).

    python tools/bench_rollout_score.py [--steps 64] [--warmup 8] [--repeats 5] [--precision bf16] [--out profiles/rollout_score.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pbml_mantle_convection_amd import _lib as L  # noqa: E402
from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet  # noqa: E402
from pbml_mantle_convection_amd.rollout import EnsembleRollout, normalise_params, synthetic_ensemble  # noqa: E402

H, W = 128, 506
VARIANTS = ("off", "idle", "staggered", "burst", "host_loop")
DUE_EVERY_STEPS = 10
BYTES_PER_DUE = 6 * H * W * 4


def parameters(B):
    """B members spread over the dataset's parameter ranges."""
    f = (np.arange(B) + 0.5) / B
    return np.stack([0.5 + 6.0 * f, 10.0 ** (6.2 + 3.0 * f), 10.0 ** (0.2 + 1.6 * f[::-1])], 1)


def timed(fn, steps):
    fn.start()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps            # ms per rollout step


def truth_times(variant, B, cap, dt):
    """[B, cap] f64: member m's k-th time, in units of its own mean step."""
    k, m = np.arange(cap)[None, :], np.arange(B)[:, None]
    if variant == "idle":
        return np.full((B, cap), 1e9) + k
    shift = (m % DUE_EVERY_STEPS) if variant in ("staggered", "host_loop") else 5
    return (DUE_EVERY_STEPS * k + shift + 0.5) * np.asarray(dt, dtype=np.float64)[:, None]


def host_scores(T, truth):
    """The notebook's figures of one member in torch, f64 on the device: MAE, max error, Pearson r, profile MAE, the two means."""
    a, b = T.double(), truth.double()
    da, db = a - a.mean(), b - b.mean()
    return torch.stack([(a - b).abs().mean(), (a - b).abs().max(), (da * db).sum() / torch.sqrt((da * da).sum() * (db * db).sum()),
                        (a.mean(1) - b.mean(1)).abs().mean(), a.mean(), b.mean()])


class Ensemble:
    def __init__(self, m, B, dev, variant, steps, dt=None):
        T0, xc, yc = synthetic_ensemble(B, H, W, seed=B)
        p = parameters(B)
        self.B, self.variant, self.dev = B, variant, dev
        on = variant in ("idle", "staggered", "burst")
        cap = steps // DUE_EVERY_STEPS + 2
        self.ro = EnsembleRollout(m, dev, use_graph=True, score_capacity=cap if on else 0)
        self.args = (torch.from_numpy(T0), xc, yc, yc, p[:, 0], p[:, 1], p[:, 2], normalise_params(p))
        self.truth = None
        if variant != "off":
            fields = synthetic_ensemble(B * cap, H, W, seed=B + 1)[0].reshape(B, cap, H, W)
            self.truth = dict(T=torch.from_numpy(fields), t=torch.from_numpy(truth_times(variant, B, cap, dt)), n=None)
        if variant == "host_loop":
            self.truth_dev = self.truth["T"].to(dev)
            self.table = torch.full((B, cap, 6), float("nan"), dtype=torch.float64, device=dev)
        self.start()

    def start(self):
        self.ro.reset(*self.args, **(dict(truth=self.truth) if self.ro.score_capacity else {}))
        self.nxt = [0] * self.B

    def __call__(self, steps):
        if self.variant != "host_loop":
            self.out = self.ro.run(steps)
            return
        tt, cap = self.truth["t"].numpy(), self.truth["t"].shape[1]
        for _ in range(steps):
            self.out = self.ro.run(1)
            t = self.out["t"].cpu().numpy()                   # the host read of the clocks
            for m in range(self.B):
                while self.nxt[m] < cap and tt[m, self.nxt[m]] <= t[m]:
                    self.table[m, self.nxt[m]] = host_scores(self.out["T"][m, 0], self.truth_dev[m, self.nxt[m]])
                    self.nxt[m] += 1

    def scored(self):
        if self.variant == "host_loop":
            return list(self.nxt)
        return self.out["score"]["scored"].cpu().tolist() if self.out["score"] is not None else None

    def finite(self):
        return bool(torch.isfinite(self.out["T"]).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 8])
    ap.add_argument("--only", type=str, default=None, choices=VARIANTS)
    ap.add_argument("--precision", type=str, default="bf16", choices=["fp32", "bf16", "mixed"])
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "rollout_score.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    torch.manual_seed(0)
    m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True).to(dev)
    m.set_precision(a.precision)
    variants = (a.only,) if a.only else VARIANTS
    runs = {}
    for B in a.batches:
        # the members' own time steps, from a few steps without the feature: the truth times are multiples of them
        probe = Ensemble(copy.deepcopy(m), B, dev, "off", a.steps)
        probe(a.warmup)
        dt = probe.out["hist"][:, :, 1].mean(0).cpu().numpy()
        if "off" in variants:
            runs[f"off_B{B}"] = probe
        for v in variants:
            if v != "off":                            # one copy of the network per captured step
                runs[f"{v}_B{B}"] = Ensemble(copy.deepcopy(m), B, dev, v, a.steps, dt)
    for r in runs.values():
        timed(r, a.warmup)                            # captures the step and warms every shape
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):                        # alternate, so that a drift of the box hits all alike
        for k, r in runs.items():
            ms[k].append(timed(r, a.steps))
    res = {"workload": "newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros + advection-diffusion step, one captured rollout step",
           "grid": [H, W], "precision": a.precision, "steps": a.steps, "repeats": a.repeats, "due_every_steps": DUE_EVERY_STEPS,
           "bytes_per_due_snapshot": BYTES_PER_DUE}
    for k, r in runs.items():
        if not r.finite():
            raise RuntimeError(f"{k}: non-finite temperature")
        med = statistics.median(ms[k])
        res[k] = {"members": r.B, "variant": r.variant, "ms_per_step": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "min_max_ms": [round(min(ms[k]), 4), round(max(ms[k]), 4)], "member_steps_per_s": round(r.B / med * 1e3, 1)}
        sc = r.scored()
        if sc is not None:                            # of the last window
            res[k]["scored_per_member"] = [int(min(sc)), int(max(sc))]
            res[k]["scored_total"] = int(sum(sc))
    for B in a.batches:
        if f"off_B{B}" in res:
            off = res[f"off_B{B}"]["median_ms"]
            for v in variants:
                if v != "off":
                    e = res[f"{v}_B{B}"]
                    e["ms_over_off"] = round(e["median_ms"] - off, 4)
                    if e.get("scored_total"):
                        e["us_per_due_snapshot"] = round((e["median_ms"] - off) * a.steps / e["scored_total"] * 1e3, 2)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()

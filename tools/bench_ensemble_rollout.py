#!/usr/bin/env python3
"""Member-steps per second of the ensemble rollout against a loop of batch-1 TS calls.

The deployed configuration (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, 128 x 506, bf16, seeded weights and fields):
`EnsembleRollout(use_graph=True)` at B = 1, 8 and 32, and `TS(use_graph=True, ts=--ts)` called at batch 1 -- the way a study
loops over simulations without this module; TS is untouched by it, so that loop is the parent's figure -- in one process,
alternating --repeats times so that all see the same box in the same state.  A timed window is --steps rollout steps (TS:
--steps / --ts forward calls) between two device events, ended by a synchronise.  Prints one JSON line and writes it to --out.

    python tools/bench_ensemble_rollout.py [--steps 64] [--warmup 8] [--repeats 5] [--precision bf16] [--out profiles/ensemble_rollout.json]
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
from pbml_mantle_convection_amd.pytorch_networks_convae import ADNet, NewFluidNet, TS  # noqa: E402
from pbml_mantle_convection_amd.rollout import EnsembleRollout, normalise_params, synthetic_ensemble  # noqa: E402

H, W = 128, 506


def parameters(B):
    """B members spread over the dataset's parameter ranges."""
    f = (np.arange(B) + 0.5) / B
    return np.stack([0.5 + 6.0 * f, 10.0 ** (6.2 + 3.0 * f), 10.0 ** (0.2 + 1.6 * f[::-1])], 1)


def timed(fn, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps            # ms per rollout step


class Ensemble:
    def __init__(self, m, B, dev):
        T0, xc, yc = synthetic_ensemble(B, H, W, seed=B)
        p = parameters(B)
        self.B = B
        self.ro = EnsembleRollout(m, dev, use_graph=True)
        self.ro.reset(torch.from_numpy(T0), xc, yc, yc, p[:, 0], p[:, 1], p[:, 2], normalise_params(p))

    def __call__(self, steps):
        self.out = self.ro.run(steps)

    def finite(self):
        return bool(torch.isfinite(self.out["T"]).all())


class Batch1Loop:
    """TS at batch 1 with its own captured step: `ts` steps per forward call, every step's T and dt cloned, as TS does."""

    def __init__(self, m, dev, ts):
        T0, xc, yc = synthetic_ensemble(1, H, W, seed=1)
        p = parameters(1)
        nd = normalise_params(p)
        self.B, self.ts_steps = 1, ts
        self.ts = TS(m, ADNet(dev), dev, ts=ts, net="newfluidnet", use_graph=True)
        g = lambda a: torch.from_numpy(a).view(1, 1, H, W)  # noqa: E731
        s = lambda v: torch.tensor(float(v))  # noqa: E731
        self.T = torch.from_numpy(T0).to(dev)
        self.args = (None, None, g(yc), s(nd[0, 0]).view(1, 1, 1, 1), s(nd[0, 1]).view(1, 1, 1, 1), s(nd[0, 2]).view(1, 1, 1, 1),
                     s(p[0, 0]), s(p[0, 1]), s(p[0, 2]), g(xc), g(yc))

    def __call__(self, steps):
        for _ in range(max(1, steps // self.ts_steps)):
            x, *_ = self.ts(self.T, *self.args)
            self.T = x[self.ts_steps]

    def finite(self):
        return bool(torch.isfinite(self.T).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ts", type=int, default=8, help="steps per TS.forward call of the batch-1 loop (the reference's default)")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--precision", type=str, default="bf16", choices=["fp32", "bf16", "mixed"])
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "ensemble_rollout.json"))
    a = ap.parse_args()
    if a.steps % a.ts:
        raise SystemExit("--steps must be a multiple of --ts")
    dev = torch.device("cuda", 0)
    L.load()
    torch.manual_seed(0)
    m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True).to(dev)
    m.set_precision(a.precision)
    # one copy of the network per captured step: an engine re-plans its buffers when the batch size changes
    runs = {"ts_batch1_loop": Batch1Loop(copy.deepcopy(m), dev, a.ts)}
    for B in a.batches:
        runs[f"ensemble_B{B}"] = Ensemble(copy.deepcopy(m), B, dev)
    for r in runs.values():
        timed(r, max(a.warmup, a.ts))                 # captures the step and warms every shape
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):                        # alternate, so that a drift of the box hits all alike
        for k, r in runs.items():
            ms[k].append(timed(r, a.steps))
    res = {"workload": "newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros + advection-diffusion step, one captured rollout step",
           "grid": [H, W], "precision": a.precision, "steps": a.steps, "repeats": a.repeats, "ts_per_forward": a.ts}
    for k, r in runs.items():
        if not r.finite():
            raise RuntimeError(f"{k}: non-finite temperature")
        med = statistics.median(ms[k])
        rate = [r.B / v * 1e3 for v in ms[k]]
        res[k] = {"members": r.B, "ms_per_step": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "spread_ms": round(max(ms[k]) - min(ms[k]), 4), "member_steps_per_s": round(r.B / med * 1e3, 1),
                  "member_steps_per_s_min_max": [round(min(rate), 1), round(max(rate), 1)]}
    base = res["ts_batch1_loop"]
    for B in a.batches:
        e = res[f"ensemble_B{B}"]
        e["speedup_vs_batch1_loop"] = round(e["member_steps_per_s"] / base["member_steps_per_s"], 3)
        # the slowest ensemble repeat against the fastest loop repeat: > 1 means the gain exceeds the run-to-run spread
        e["speedup_worst_case"] = round(e["member_steps_per_s_min_max"][0] / base["member_steps_per_s_min_max"][1], 3)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the ensemble rollout's statistics: milliseconds per captured step with the options off, with profiles=True, and
with profiles plus timed saves (save_every chosen per member so that about one step in ten saves).

The method of tools/bench_ensemble_rollout.py: the deployed configuration (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros,
128 x 506, bf16, seeded weights and fields), `EnsembleRollout(use_graph=True)` at B = 32 and 8, in one process, alternating
--repeats times so that all variants see the same box in the same state.  A timed window is --steps rollout steps between
two device events, ended by a synchronise.  "off" issues the launches of the rollout without the options.  Prints one JSON
line and writes it to --out.  --only VARIANT --batches B runs one variant alone (for a kernel trace).

    python tools/bench_ensemble_stats.py [--steps 64] [--warmup 8] [--repeats 5] [--precision bf16] [--out profiles/ensemble_stats.json]
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
VARIANTS = ("off", "profiles", "profiles_saves")
SAVE_EVERY_STEPS = 10


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
    def __init__(self, m, B, dev, variant, steps, dt=None):
        T0, xc, yc = synthetic_ensemble(B, H, W, seed=B)
        p = parameters(B)
        self.B, self.variant = B, variant
        saves = variant == "profiles_saves"
        cap = steps // SAVE_EVERY_STEPS + 2 if saves else 0
        self.ro = EnsembleRollout(m, dev, use_graph=True, profiles=variant != "off", save_capacity=cap)
        kw = dict(save_every=SAVE_EVERY_STEPS * dt) if saves else {}
        self.ro.reset(torch.from_numpy(T0), xc, yc, yc, p[:, 0], p[:, 1], p[:, 2], normalise_params(p), **kw)

    def __call__(self, steps):
        self.out = self.ro.run(steps)

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
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "ensemble_stats.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    torch.manual_seed(0)
    m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True).to(dev)
    m.set_precision(a.precision)
    variants = (a.only,) if a.only else VARIANTS
    runs = {}
    for B in a.batches:
        # the members' own time steps, from a few steps without the options: the saving variant saves every tenth of them
        probe = Ensemble(copy.deepcopy(m), B, dev, "off", a.steps)
        probe(a.warmup)
        dt = probe.out["hist"][:, :, 1].mean(0).cpu()
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
           "grid": [H, W], "precision": a.precision, "steps": a.steps, "repeats": a.repeats, "save_every_steps": SAVE_EVERY_STEPS}
    for k, r in runs.items():
        if not r.finite():
            raise RuntimeError(f"{k}: non-finite temperature")
        med = statistics.median(ms[k])
        res[k] = {"members": r.B, "variant": r.variant, "ms_per_step": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "min_max_ms": [round(min(ms[k]), 4), round(max(ms[k]), 4)], "member_steps_per_s": round(r.B / med * 1e3, 1)}
        if r.out["profiles"] is not None:
            res[k]["profile_count"] = int(r.out["profiles"]["count"].min())
        if r.out["timed"] is not None:                # of the last window
            res[k]["saves_per_member"] = [int(r.out["timed"]["count"].min()), int(r.out["timed"]["count"].max())]
            res[k]["missed"] = int(r.out["timed"]["missed"].sum())
    for B in a.batches:
        if f"off_B{B}" in res:
            for v in variants:
                if v != "off":
                    res[f"{v}_B{B}"]["cost_vs_off"] = round(res[f"{v}_B{B}"]["median_ms"] / res[f"off_B{B}"]["median_ms"] - 1.0, 4)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()

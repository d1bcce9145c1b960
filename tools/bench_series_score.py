#!/usr/bin/env python3
"""Cost of series scoring: a store of --snapshots synthetic snapshots (evaluate.synthetic_series) scored by the deployed
configuration (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, 128 x 506, bf16, seeded weights), batch 32.

  (a) "score":   SeriesScorer(use_graph=True).score(store): gather -> network -> row pass -> finalize per captured step;
  (b) "forward": the same scorer with the two scoring launches left out of the step (gather -> network): (a) - (b) is what
                 scoring adds to a step;
  (c) "loop":    the way open before SeriesScorer existed: per snapshot one batch-1 TS(net, ADNet, ts=1, use_graph=True) call,
                 the notebook's torch expressions for the ten metrics and ONE device-to-host read (on --loop_snapshots
                 snapshots: the rate does not depend on their number).

The method of tools/bench_ensemble_stats.py: one process, variants alternating --repeats times so that all see the same box in
the same state; a timed window is one whole pass between two device events, ended by a synchronise; (a) and (b) both include
the copy of the store into the scorer's buffers.  Prints one JSON line and writes it to --out.

    python tools/bench_series_score.py [--snapshots 2048] [--loop_snapshots 128] [--repeats 5] [--only VARIANT] [--precision bf16] [--out profiles/series_score.json]
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
from pbml_mantle_convection_amd.evaluate import SeriesScorer, SeriesStore, previous_snapshots, synthetic_series  # noqa: E402
from pbml_mantle_convection_amd.pytorch_networks_convae import ADNet, NewFluidNet, TS  # noqa: E402
from pbml_mantle_convection_amd.rollout import normalise_params  # noqa: E402
from pbml_mantle_convection_amd.scaler import velocity_scaler  # noqa: E402

H, W = 128, 506
DISTINCT = 64


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                    # ms per pass


def mass(u, v):
    """get_mass(..., bc=False) of the notebook on [1,1,H,W] fields."""
    return (0.5 * (u[..., 1:-1, 2:] - u[..., 1:-1, :-2]) + 0.5 * (v[..., 2:, 1:-1] - v[..., :-2, 1:-1])).abs().mean()


class Loop:
    """(c): TS at batch 1 per snapshot, metrics as torch expressions in the scaled space, one read per snapshot."""

    def __init__(self, m, arrays, dev, n):
        self.ts = TS(m, ADNet(dev), dev, ts=1, net="newfluidnet", use_graph=True)
        self.dev, self.n, self.a = dev, n, arrays
        self.T, self.u, self.v = (torch.from_numpy(arrays[k][:n]).to(dev).view(n, 1, 1, H, W) for k in "Tuv")
        self.xc, self.yc = (torch.from_numpy(arrays[k]).view(1, 1, H, W) for k in ("xc", "yc"))
        paras = np.stack([arrays["raq"], arrays["fkt"], arrays["fkp"]], 1)
        self.paras, self.nd = paras, normalise_params(paras)
        self.scale = velocity_scaler(paras[:, 0], paras[:, 1], paras[:, 2])
        self.rows = []

    def __call__(self):
        a, rows = self.a, []
        for n in range(self.n):
            s, pv = int(a["sim"][n]), int(a["prev"][n])
            par = [torch.tensor(float(x)) for x in self.paras[s]]
            nd = [torch.tensor(float(x)).view(1, 1, 1, 1) for x in self.nd[s]]
            _, _, up, vp, _, _ = self.ts(self.T[n], None, None, self.yc, nd[0], nd[1], nd[2], par[0], par[1], par[2], self.xc, self.yc)
            sc = float(self.scale[s])
            ut, vt, up, vp = self.u[n] / sc, self.v[n] / sc, up / sc, vp / sc
            ub, vb = (self.u[pv] / sc, self.v[pv] / sc) if pv >= 0 else (ut, vt)
            row = torch.stack([(ut - up).abs().mean(), (vt - vp).abs().mean(), (ut - ub).abs().mean(), (vt - vb).abs().mean(),
                               ut.abs().max(), vt.abs().max(), (ut - up).abs().max(), (vt - vp).abs().max(), mass(up, vp), mass(ut, vt)])
            rows.append(row.tolist())             # the one device-to-host read of this snapshot
        self.rows = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshots", type=int, default=2048)
    ap.add_argument("--loop_snapshots", type=int, default=128)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", type=str, default=None, choices=["score", "forward", "loop"], help="one variant alone (for a kernel trace)")
    ap.add_argument("--precision", type=str, default="bf16", choices=["fp32", "bf16", "mixed"])
    ap.add_argument("--out", type=str, default=os.path.join("profiles", "series_score.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    torch.manual_seed(0)
    m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True).to(dev)
    m.set_precision(a.precision)
    if a.snapshots % DISTINCT:
        raise SystemExit(f"--snapshots must be a multiple of {DISTINCT}")
    arrays = synthetic_series(DISTINCT, H, W, seed=0)       # distinct fields, repeated: the cost does not depend on the values
    reps = a.snapshots // DISTINCT
    arrays.update({k: np.tile(arrays[k], (reps, 1, 1)) for k in "Tuv"}, sim=np.tile(arrays["sim"], reps))
    arrays["prev"] = previous_snapshots(arrays["sim"])
    store = SeriesStore(**arrays, device=dev)
    steps = -(-a.snapshots // a.batch)
    out = {}
    scorers = {k: SeriesScorer(copy.deepcopy(m), dev, batch=a.batch, use_graph=True, scoring=k == "score") for k in ("score", "forward")}
    runs = {k: (lambda k=k: out.__setitem__(k, scorers[k].score(store))) for k in scorers}
    runs["loop"] = Loop(copy.deepcopy(m), arrays, dev, min(a.loop_snapshots, a.snapshots))
    if a.only:
        runs = {a.only: runs[a.only]}
    for r in runs.values():
        timed(r)                                  # captures the steps and warms every shape
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):                    # alternate, so that a drift of the box hits all alike
        for k, r in runs.items():
            ms[k].append(timed(r))
    if "score" in runs:
        table = out["score"]["table"].cpu().numpy()
        if not np.isfinite(table[:, [0, 1, 4, 5, 6, 7, 8, 9]]).all():
            raise RuntimeError("non-finite scores")
    res = {"workload": "newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, series scoring, one captured step = gather + forward + row pass + finalize",
           "grid": [H, W], "precision": a.precision, "batch": a.batch, "snapshots": a.snapshots, "steps_per_pass": steps,
           "loop_snapshots": min(a.loop_snapshots, a.snapshots), "repeats": a.repeats}
    for k in runs:
        med = statistics.median(ms[k])
        n = res["loop_snapshots"] if k == "loop" else a.snapshots
        res[k] = {"ms_per_pass": [round(v, 3) for v in ms[k]], "median_ms": round(med, 3), "min_max_ms": [round(min(ms[k]), 3), round(max(ms[k]), 3)],
                  "snapshots_per_s": round(n / med * 1e3, 1)}
        if k != "loop":
            res[k]["ms_per_step"] = round(med / steps, 4)
    if not a.only:
        res["scoring_ms_per_step"] = round(res["score"]["ms_per_step"] - res["forward"]["ms_per_step"], 4)
        res["scoring_cost_vs_forward"] = round(res["score"]["median_ms"] / res["forward"]["median_ms"] - 1.0, 4)
        res["speedup_vs_loop"] = round(res["score"]["snapshots_per_s"] / res["loop"]["snapshots_per_s"], 2)
        # the loop's MAE of u on its snapshots beside the scorer's (bf16 forwards at batch 1 and 32: close, not equal)
        loop_rows = np.asarray(runs["loop"].rows)
        res["mae_u_loop_vs_score"] = [float(loop_rows[:, 0].mean()), float(table[:loop_rows.shape[0], 0].mean())]
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()

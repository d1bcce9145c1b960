#!/usr/bin/env python3
"""What the guarded optimizer step costs in the headline training step.

HIP-graph-captured training steps of the headline U-Net (CFG-3, built exactly as `bench.py` builds it: levels 5, c_h 16, k 5,
repeats 3, reflect, mass loss + momentum residual, batch 32 on the 506 x 506 grid, 'mixed', synthetic data) with the guard off
and with it on (max_grad_norm and skip_nonfinite both set), in one process, alternating --repeats times so that both see the same
box in the same state.  The guard-off trainer issues today's launches: its figure is `bench.py`'s.  Prints one JSON line and
writes it to --out: per mode the ms / step of every repeat, their median and spread, and the cost.

    python tools/bench_grad_guard.py [--steps 20] [--warmup 5] [--repeats 3] [--batch 32] [--precision mixed] [--clip_norm 1.0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pbml_mantle_convection_amd import _lib as L  # noqa: E402
from pbml_mantle_convection_amd.datasetio import synthetic_batch  # noqa: E402
from pbml_mantle_convection_amd.multigpu import Trainer  # noqa: E402
from pbml_mantle_convection_amd.pytorch_networks_convae import Unet  # noqa: E402


class Step:
    """One captured trainer; time(steps) replays it."""

    def __init__(self, guard, prec, B, H, W, clip, dev):
        torch.manual_seed(0)
        m = Unet(5, 10, 16, 4, dev, "gelu", "reflect", "mass", use_symm=True, repeats=3, f=5, p_pred=True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10 ** 9], gamma=0.5)
        kw = dict(max_grad_norm=clip, skip_nonfinite=True) if guard else {}
        self.tr = Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="unet", loss_type="mass",
                          lambda_mom=1e-6, precision=prec, use_graph=True, **kw)
        gVTp, uvp, scaler, paras, yc = (t.to(dev) for t in synthetic_batch(B, H, W, 1234, p_pred=True, device="cpu"))
        self.tr.train_step(gVTp, uvp, yc, paras, scaler)                # captures the step
        b = self.tr.input_buffers()
        self.args = (b["gVTp"], b["uvp"], b["yc"], b["paras"], b["scaler"])

    def time(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            out = self.tr.train_step(*self.args)
        e1.record()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out[0])):
            raise RuntimeError("non-finite loss")
        return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=[506, 506], metavar=("H", "W"))
    ap.add_argument("--precision", type=str, default="mixed", choices=["fp32", "bf16", "mixed"])
    ap.add_argument("--clip_norm", type=float, default=1.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "grad_guard_step.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    modes = ["off", "on"]
    runs = {k: Step(k == "on", a.precision, a.batch, a.size[0], a.size[1], a.clip_norm, dev) for k in modes}
    for s in runs.values():
        s.time(max(a.warmup, 1))
    ms = {k: [] for k in modes}
    for _ in range(a.repeats):                       # alternate, so that a drift of the box hits both alike
        for k in modes:
            ms[k].append(runs[k].time(a.steps))
    res = {"workload": "CFG-3 U-Net (levels 5, c_h 16, k 5, repeats 3, reflect), mass loss + momentum residual, captured "
                       "training step", "batch": a.batch, "grid": list(a.size), "precision": a.precision, "steps": a.steps,
           "repeats": a.repeats, "numel": runs["on"].tr.flat.numel, "max_grad_norm": a.clip_norm, "skip_nonfinite": True}
    for k in modes:
        med = statistics.median(ms[k])
        res[f"guard_{k}"] = {"ms_per_step": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                             "spread_ms": round(max(ms[k]) - min(ms[k]), 4), "samples_per_s": round(a.batch / med * 1e3, 1)}
    rec = runs["on"].tr.grad_guard()
    res["guard_record"] = {k: rec[k] for k in ("norm", "coef", "nonfinite", "skipped")}
    m0, m1 = res["guard_off"]["median_ms"], res["guard_on"]["median_ms"]
    res["guard_cost_ms"] = round(m1 - m0, 4)
    res["guard_cost_frac"] = round(m1 / m0 - 1.0, 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

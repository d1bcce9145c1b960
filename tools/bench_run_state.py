#!/usr/bin/env python3
"""What one state save (`--save_state 1`) costs against an epoch of the headline training step.

One HIP-graph-captured trainer of the headline U-Net (CFG-3, built exactly as `bench.py` builds it: levels 5, c_h 16, k 5,
repeats 3, reflect, mass loss + momentum residual, batch 32 on the 506 x 506 grid, 'mixed', synthetic data; 1 819 680
parameters).  Alternating --repeats times: an "epoch" of --steps replayed steps, then `Trainer.state_dict()` (three flat
buffers device -> host, the per-rank entry) and `write_state_file` (torch.save to a temporary name, os.replace) into a
temporary directory.  Prints one JSON line and writes it to --out: per repeat the epoch's ms, the state_dict ms and the file
write ms, their medians, the file's size and the save as a fraction of the epoch.

    python tools/bench_run_state.py [--steps 20] [--warmup 5] [--repeats 3] [--batch 32] [--precision mixed]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pbml_mantle_convection_amd import _lib as L  # noqa: E402
from pbml_mantle_convection_amd.datasetio import synthetic_batch  # noqa: E402
from pbml_mantle_convection_amd.multigpu import STATE_FILE, Trainer, read_state_file, write_state_file  # noqa: E402
from pbml_mantle_convection_amd.pytorch_networks_convae import Unet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, nargs=2, default=[506, 506], metavar=("H", "W"))
    ap.add_argument("--precision", type=str, default="mixed", choices=["fp32", "bf16", "mixed"])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "run_state_save.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    torch.manual_seed(0)
    m = Unet(5, 10, 16, 4, dev, "gelu", "reflect", "mass", use_symm=True, repeats=3, f=5, p_pred=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10 ** 9], gamma=0.5)
    tr = Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="unet", loss_type="mass",
                 lambda_mom=1e-6, precision=a.precision, use_graph=True, save_state=True)
    gVTp, uvp, scaler, paras, yc = (t.to(dev) for t in synthetic_batch(a.batch, a.size[0], a.size[1], 1234, p_pred=True, device="cpu"))
    tr.train_step(gVTp, uvp, yc, paras, scaler)                         # captures the step
    b = tr.input_buffers()
    args = (b["gVTp"], b["uvp"], b["yc"], b["paras"], b["scaler"])

    def epoch(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = tr.train_step(*args)
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out[0])):
            raise RuntimeError("non-finite loss")
        return (time.perf_counter() - t0) * 1e3

    epoch(max(a.warmup, 1))
    ms = {"epoch": [], "state_dict": [], "write": []}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, STATE_FILE)
        write_state_file(tr.state_dict(), path)                         # (first touch of the page cache and of pinned staging)
        for _ in range(a.repeats):
            ms["epoch"].append(epoch(a.steps))
            t0 = time.perf_counter()
            st = tr.state_dict()
            t1 = time.perf_counter()
            write_state_file(st, path)
            t2 = time.perf_counter()
            ms["state_dict"].append((t1 - t0) * 1e3)
            ms["write"].append((t2 - t1) * 1e3)
        size = os.path.getsize(path)
        back = read_state_file(path)
        if not torch.equal(back["optimizer"]["param"], tr.flat.param.cpu()) or os.listdir(d) != [STATE_FILE]:
            raise RuntimeError("the state file does not hold the trainer's parameters")
    res = {"workload": "CFG-3 U-Net (levels 5, c_h 16, k 5, repeats 3, reflect), mass loss + momentum residual, captured "
                       "training step", "batch": a.batch, "grid": list(a.size), "precision": a.precision, "steps_per_epoch": a.steps,
           "repeats": a.repeats, "numel": tr.flat.numel, "file_bytes": size}
    for k, v in ms.items():
        res[f"{k}_ms"] = {"runs": [round(x, 3) for x in v], "median": round(statistics.median(v), 3)}
    save = statistics.median([s + w for s, w in zip(ms["state_dict"], ms["write"])])
    res["save_ms"] = round(save, 3)
    res["save_over_epoch"] = round(save / res["epoch_ms"]["median"], 4)
    res["save_in_steps"] = round(save / (res["epoch_ms"]["median"] / a.steps), 3)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

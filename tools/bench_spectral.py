#!/usr/bin/env python3
"""Spectral trunk: training-step time and the two streaming kernels on their own.

Step: HIP-graph-captured training steps of the deployed NewFluidNet (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, as
`bench.py --workload newfluidnet` builds it) with spectral_conv=True at batch 32 on the 128 x 506 grid, synthetic data: ms /
step and samples / s per precision.  Run `python bench.py --workload newfluidnet` beside it for the conv trunk.

Kernels (--kernels): mc_spectral_analyze / mc_spectral_synthesize alone through the C ABI at 128 x 506 x 16 channels x 32 and
at 506 x 512 x 16 x 8, HIP-event time over --steps launches and the algorithmic TB/s (the input read once or the output
written once).  Prints one JSON line.

    python tools/bench_spectral.py [--steps 20] [--warmup 5] [--batch 32] [--precisions bf16,fp32] [--kernels]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pbml_mantle_convection_amd import _lib as L  # noqa: E402
from pbml_mantle_convection_amd.datasetio import synthetic_batch  # noqa: E402
from pbml_mantle_convection_amd.engine import spectral_tables  # noqa: E402
from pbml_mantle_convection_amd.multigpu import Trainer  # noqa: E402
from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet  # noqa: E402


def run_step(prec, B, steps, warmup, dev, spectral=True):
    torch.manual_seed(0)
    m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True, spectral_conv=spectral)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10 ** 9], gamma=0.5)
    tr = Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="newfluidnet", loss_scale=True,
                 loss_derivative=False, loss_type="mass", precision=prec, use_graph=True)
    gVTp, uvp, *_ = synthetic_batch(B, 128, 506, 1234, p_pred=True, device="cpu")
    x, y = gVTp[:, :7].contiguous().to(dev), uvp[:, :3].contiguous().to(dev)
    out = tr.train_step(x, y)                     # captures the step
    st = tr.input_buffers()
    x, y = st["gVTp"], st["uvp"]
    for _ in range(warmup - 1):
        out = tr.train_step(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        out = tr.train_step(x, y)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    loss = float(out[0])
    if not torch.isfinite(torch.tensor(loss)):
        raise RuntimeError(f"{prec}: non-finite loss")
    return {"ms_per_step": round(ms, 4), "samples_per_s": round(B / ms * 1e3, 1), "loss": loss}


def run_kernels(N, C, H, W, steps, warmup, dev):
    row, col = (torch.from_numpy(t).to(dev) for t in spectral_tables(H, W))
    slots = L.call("mc_spectral_slots", H, W)
    part = torch.empty((N, slots, C, 32, 2), device=dev)
    coef = torch.randn((N, C, 32, 2), device=dev)
    gn = torch.empty((N, slots, C, 2), device=dev)
    out = {"shape": [N, C, H, W], "slots": slots}
    for name, mc, dt in (("f32", L.MC_F32, torch.float32), ("bf16", L.MC_BF16, torch.bfloat16), ("f16", L.MC_MIX16, torch.float16)):
        x = torch.randn((N, C // 8, H, W, 8), device=dev).to(dt)
        y = torch.empty_like(x)
        st = L.stream()
        launches = {"analyze": lambda: L.call("mc_spectral_analyze", L.ptr(x), N, C, H, W, mc, L.ptr(row), L.ptr(col), L.ptr(part), st),
                    "synthesize": lambda: L.call("mc_spectral_synthesize", L.ptr(coef), N, C, H, W, mc, L.ptr(row), L.ptr(col), L.ptr(y),
                                                 None, st),
                    "synthesize+gn": lambda: L.call("mc_spectral_synthesize", L.ptr(coef), N, C, H, W, mc, L.ptr(row), L.ptr(col),
                                                    L.ptr(y), L.ptr(gn), st)}
        for kname, fn in launches.items():
            for _ in range(warmup):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / steps
            out[f"{kname}_{name}"] = {"us": round(us, 2), "TBps": round(x.numel() * x.element_size() / (us * 1e-6) / 1e12, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precisions", type=str, default="bf16,fp32")
    ap.add_argument("--kernels", action="store_true", help="time the two streaming kernels alone instead of the training step")
    ap.add_argument("--conv-trunk", action="store_true", help="the same step with the conv trunk (spectral_conv=False)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    if a.kernels:
        res = {"workload": "spectral streaming kernels, stand-alone", "steps": a.steps,
               "trunk_level0": run_kernels(32, 16, 128, 506, a.steps, max(a.warmup, 1), dev),
               "large": run_kernels(8, 16, 506, 512, a.steps, max(a.warmup, 1), dev)}
    else:
        res = {"workload": "newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, mass loss, captured training step, "
                           + ("conv trunk" if a.conv_trunk else "spectral_conv=True"),
               "batch": a.batch, "grid": [128, 506], "steps": a.steps}
        for prec in a.precisions.split(","):
            res[prec] = run_step(prec, a.batch, a.steps, max(a.warmup, 1), dev, spectral=not a.conv_trunk)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

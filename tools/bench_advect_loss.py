#!/usr/bin/env python3
"""What the advection loss (-ad 1, DESIGN.md §9 "Advection loss") costs in the deployed network's training step.

HIP-graph-captured training steps of the deployed NewFluidNet (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros: mass loss,
scaled L1, batch 16 on the 128 x 506 grid, bf16, synthetic fields in the NewADDataset channel order) without the term
(model_AD = None: today's graph, launch for launch) and with it (ADNet(CN_max = 2e4)), in one process, alternating --repeats
times so that both see the same box in the same state.  Then the two new entry points alone, each captured --inner times in a
graph of its own and replayed (so that launch gaps of the host do not count): mc_advect_loss_dt (two small kernels) and
mc_advect_loss (one).  Writes profiles/advect_loss.json (or --out) and prints it as one JSON line.

    python tools/bench_advect_loss.py [--steps 20] [--warmup 5] [--repeats 3] [--batch 16] [--precision bf16] [--out PATH]
"""
import argparse
import ctypes as C
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
from pbml_mantle_convection_amd.pytorch_networks_convae import ADNet, NewFluidNet  # noqa: E402

H, W = 128, 506


def batch(B, dev):
    """x (xc/4, yc/4, log10 eta/8, nd0, nd1, nd2, T), truth (u, v, p), scaler: the item layout of NewADDataset."""
    g, uvp, scaler, *_ = synthetic_batch(B, H, W, 1234, p_pred=True, device="cpu")
    x = torch.stack([g[:, 0] / 4, g[:, 1] / 4, g[:, 6], g[:, 3], g[:, 4], g[:, 5], g[:, 7]], 1)
    return x.contiguous().to(dev), uvp[:, :3].contiguous().to(dev), scaler.float().to(dev)


class Step:
    """One captured trainer; time(steps) replays it."""

    def __init__(self, advect, prec, B, dev):
        torch.manual_seed(0)
        m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10 ** 9], gamma=0.5)
        self.tr = Trainer(m, ADNet(device=0, CN_max=2e4) if advect else None, None, None, None, None, opt, sch, 0, 1, "/tmp/",
                          p_pred=True, network="newfluidnet", loss_scale=True, loss_derivative=False, loss_type="mass",
                          precision=prec, use_graph=True, drop_seed=1234)
        x, y, s = batch(B, dev)
        self.tr.train_step(x, y, scaler=s if advect else None)                       # captures the step
        st = self.tr.input_buffers()
        self.x, self.y, self.s = st["gVTp"], st["uvp"], st["scaler"]

    def time(self, steps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            out = self.tr.train_step(self.x, self.y, scaler=self.s)
        e1.record()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(out[:6]).all()):
            raise RuntimeError("non-finite loss")
        self.out = [float(v) for v in out[:6].tolist()]
        return e0.elapsed_time(e1) / steps


def time_graph(fn, inner, replays, warmup=3):
    """us per call of fn, captured `inner` times in one graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    for _ in range(warmup):
        g.replay()
    out = []
    for _ in range(replays):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return out


def kernels(B, dev, inner, replays):
    x, uvp, s = batch(B, dev)
    y = torch.randn((B, 3, H, W), device=dev) * 0.1
    gy = torch.zeros_like(y)
    dt, ws = torch.zeros(B, device=dev), torch.zeros(L.ADVECT_WS_PER_ITEM * B, dtype=torch.int32, device=dev)
    sums = torch.zeros(L.LOSS_SLOTS, dtype=torch.float64, device=dev)
    d = L.LossDesc(B, H, W, 1, 1, 1, 0, 0, 0.0, 126.0, 1.0, -2)
    HW = H * W

    def f_dt():
        L.call("mc_advect_loss_dt", L.ptr(uvp), 3, L.ptr(x), 7, L.ptr(s), B, H, W, 2e4, L.ptr(ws), L.ptr(dt), L.stream())

    def f_loss():
        L.call("mc_advect_loss", C.byref(d), y.data_ptr(), y.data_ptr() + 4 * HW, 3 * HW, L.ptr(uvp), L.ptr(x), 7, L.ptr(s), L.ptr(dt),
               L.ptr(sums), gy.data_ptr(), gy.data_ptr() + 4 * HW, L.stream())
    t_dt = time_graph(f_dt, inner, replays)
    t_loss = time_graph(f_loss, inner, replays)
    plane = B * HW * 4
    mb_dt, mb_loss = 3 * plane / 1e6, 11 * plane / 1e6

    def row(t, mb):
        med = statistics.median(t)
        return {"us": [round(v, 2) for v in t], "median_us": round(med, 2), "mb_moved": round(mb, 1),
                "tb_per_s": round(mb / med, 3)}                        # (MB per us)
    return {"mc_advect_loss_dt": row(t_dt, mb_dt), "mc_advect_loss": row(t_loss, mb_loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--precision", type=str, default="bf16", choices=["fp32", "bf16", "mixed"])
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "advect_loss.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L.load()
    runs = {ad: Step(ad, a.precision, a.batch, dev) for ad in (False, True)}
    for s in runs.values():
        s.time(max(a.warmup, 1))
    ms = {ad: [] for ad in runs}
    for _ in range(a.repeats):                       # alternate, so that a drift of the box hits both alike
        for ad in runs:
            ms[ad].append(runs[ad].time(a.steps))
    res = {"workload": "newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, mass loss, captured training step", "batch": a.batch,
           "grid": [H, W], "precision": a.precision, "steps": a.steps, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    for ad in runs:
        med = statistics.median(ms[ad])
        res[f"ad_{int(ad)}"] = {"ms_per_step": [round(v, 4) for v in ms[ad]], "median_ms": round(med, 4),
                                "spread_ms": round(max(ms[ad]) - min(ms[ad]), 4), "samples_per_s": round(a.batch / med * 1e3, 1),
                                "out6": runs[ad].out}
    res["advect_cost_ms"] = round(res["ad_1"]["median_ms"] - res["ad_0"]["median_ms"], 4)
    res["advect_cost_frac"] = round(res["ad_1"]["median_ms"] / res["ad_0"]["median_ms"] - 1.0, 4)
    res["kernels"] = kernels(a.batch, dev, a.inner, max(a.repeats, 3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fw:
        json.dump(res, fw, indent=1)
        fw.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

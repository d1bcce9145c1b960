#!/usr/bin/env python3
"""Epoch loop measurement (DESIGN §9 "Resident epoch loop"): seconds per training step over one epoch of the deployed
NewFluidNet (-net newfluidnet -l 5 -f 16 -r 6 -k 5 -p zeros, batch 16, bf16, use_graph) on a synthetic shard tree in the
reference's layout at 128 x 506, fed (a) by the host DataLoader (items built on the host in fp64, shipped over PCIe, copied
into the captured step's buffers) and (b) by ResidentLoaders (the batch assembled inside the captured step), alternating.
Next to both: the per-step time of `bench.py --workload newfluidnet --batch 16` (one batch resident in HBM: the floor), the
stand-alone time of the loader's assembly launch, and the line of tools/bench_assemble.py.

usage: tools/bench_resident_epoch.py [--items 320] [--rounds 3] [--out profiles/resident_epoch.json]"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pbml_mantle_convection_amd.datasetio import NewADDataset  # noqa: E402
from pbml_mantle_convection_amd.multigpu import Trainer, prepare_dataloader, resident_loader  # noqa: E402
from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet  # noqa: E402

H, W, B = 128, 506, 16


def write_tree(root, items, sims=4, n_init=8, n_cv=32):
    g = torch.Generator().manual_seed(1)
    yy = torch.linspace(0, 1, H, dtype=torch.float64).view(H, 1).expand(H, W).contiguous()
    xx = torch.linspace(0, 4, W, dtype=torch.float64).view(1, W).expand(H, W).contiguous()
    table = []
    for s in range(sims + 1):
        an, n = ("cv", n_cv) if s == sims else ("train", items // sims)
        raq, fkt, fkp = 1.0 + s, 10.0 ** (6.5 + 0.5 * s), 10.0 ** (0.3 + 0.3 * s)
        table.append((s, an, raq, fkt, fkp, 0.0, 0.0, 0))
        d = os.path.join(root, an, f"sim_{s}")
        os.makedirs(d)
        torch.save(torch.arange(3 * n + 5, dtype=torch.float64) * 1e-3, os.path.join(d, "times.pt"))
        torch.save(xx, os.path.join(d, "xc.pt"))
        torch.save(yy, os.path.join(d, "yc.pt"))
        for suffix, m in (("_select", n), ("_select_init", n_init)):
            T = (1.0 - yy).float().expand(m, 1, H, W) + 0.1 * torch.rand((m, 1, H, W), generator=g)
            torch.save(T.clamp(0.0, 1.35), os.path.join(d, f"e1_Tprev_data{suffix}.pt"))
            for k in "uvp":
                torch.save(torch.randn((m, 1, H, W), generator=g), os.path.join(d, f"e1_{k}prev_data{suffix}.pt"))
            torch.save(torch.arange(m) * (3 if suffix == "_select" else 1) + 1, os.path.join(d, f"e1_i_vec{suffix}.pt"))
    torch.save(table, os.path.join(root, "sims.pt"))


def trainer(train, cv):
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    m = NewFluidNet(5, 7, 16, 3, dev, "gelu", "zeros", "mass", use_symm=True, repeats=6, f=5, p_pred=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[10 ** 9], gamma=0.5)
    return Trainer(m, None, train, cv, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="newfluidnet", loss_scale=True,
                   loss_type="mass", precision="bf16", use_graph=True)


def host_epoch(tr):
    """The training half of Trainer._run_epoch on the DataLoader, without its prints."""
    acc = torch.zeros(8, dtype=torch.float64, device=tr.device)
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    for data in tr.train_data:
        gVTp, uvp, scaler, paras, yc = tr._unpack(data)
        acc += tr._run_batch(gVTp, uvp, scaler, True, paras=paras, yc=yc, sync=False).double()
        n += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, n


def resident_epoch(tr, epoch):
    acc = torch.zeros(8, dtype=torch.float64, device=tr.device)
    ld = tr.train_data
    ld.start_epoch(epoch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(len(ld)):
        acc += tr.resident_step(ld, True).double()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(ld), len(ld)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=320)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "resident_epoch.json"))
    a = ap.parse_args()
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "config": f"NewFluidNet levels 5, c_h 16, k 5, repeats 6, zeros, symmetric, mass loss; {H}x{W}, batch {B}, bf16, HIP-graph "
                     f"replay; {a.items} train items in 4 simulations, f32 shard files"}
    with tempfile.TemporaryDirectory() as root:
        write_tree(root, a.items)
        kw = dict(scale=True, load=False, p_pred=True, debug=False, noise=0.0)
        ds = {(an, init): NewADDataset(root, an, is_init=init, **kw) for an in ("train", "cv") for init in (False, True)}
    host = trainer(prepare_dataloader(ds["train", False], B, 1, 0), None)
    loaders = [resident_loader(ds[an, False], ds[an, True], B, 0, 1, len(ds[an, False]), seed=0) for an in ("train", "cv")]
    resi = trainer(*loaders)
    host_epoch(host)                                         # capture and warm both before the timed rounds
    resident_epoch(resi, 0)
    rows = []
    for r in range(a.rounds):
        h, nh = host_epoch(host)
        d, nd = resident_epoch(resi, r + 1)
        rows.append(dict(host_dataloader_s_per_step=h, host_steps=nh, resident_s_per_step=d, resident_steps=nd))
        print(json.dumps(rows[-1]), flush=True)
    res["rounds"] = rows
    res["host_dataloader_ms_per_step"] = 1e3 * statistics.median(x["host_dataloader_s_per_step"] for x in rows)
    res["resident_ms_per_step"] = 1e3 * statistics.median(x["resident_s_per_step"] for x in rows)
    # the assembly launch (+ cursor advance) alone
    ld = loaders[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ld.launch()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        ld.launch()
    e1.record()
    torch.cuda.synchronize()
    res["assembly_launch_us"] = e0.elapsed_time(e1) * 1e3 / 50
    ld.start_epoch(0)
    del host, resi
    torch.cuda.empty_cache()
    # the floor: the same step on one batch that already sits in HBM
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "newfluidnet", "--gpus", "1", "--batch", str(B),
                          "--steps", "40", "--warmup", "10"], capture_output=True, text=True, check=True).stdout
    res["bench_floor_ms_per_step"] = json.loads(out.strip().split("\n")[-1])["ms_per_step"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_assemble.py"), "--size", str(H), str(W), "--batch", str(B)],
                         capture_output=True, text=True, check=True).stdout
    res["bench_assemble"] = out.strip().split("\n")
    res["resident_minus_floor_ms"] = res["resident_ms_per_step"] - res["bench_floor_ms_per_step"]
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

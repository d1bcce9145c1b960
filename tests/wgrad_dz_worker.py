"""Child process of tests/test_hip_wgrad_dz.py: one training step of a two-level U-Net (c_h 16, B = 2, "mixed", lambda_mom =
1e-6) per configuration, eager and captured, under the MANTLE_WGRAD_DZ setting of the environment it was started with.
usage: wgrad_dz_worker.py out.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np
import torch

DEV = "cuda:0"
# name -> (H, W, MANTLE_FUSE).  At 40 x 48 no input-gradient launch carries the dz epilogue by default (the row-reuse kernel
# needs 140 columns); MANTLE_FUSE=2 puts it on the wide-tile kernel's launches.
CONFIGS = {"narrow": (40, 48, None), "narrow_fuse2": (40, 48, "2"), "wide": (40, 150, None)}


def trainer(use_graph):
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import Unet
    torch.manual_seed(3)
    m = Unet(2, 10, 16, 4, torch.device(DEV), "gelu", "reflect", "mass", use_symm=True, repeats=2, f=5, p_pred=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1000], gamma=0.5)
    return Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="unet", loss_type="mass",
                   lambda_mom=1e-6, precision="mixed", use_graph=use_graph)


def main(out):
    from pbml_mantle_convection_amd.datasetio import synthetic_batch
    res = {}
    for name, (H, W, fuse) in CONFIGS.items():
        if fuse is None:
            os.environ.pop("MANTLE_FUSE", None)
        else:
            os.environ["MANTLE_FUSE"] = fuse
        gVTp, uvp, scaler, paras, yc = [t.to(DEV) for t in synthetic_batch(2, H, W, 5, p_pred=True, device="cpu")]
        tr = trainer(False)
        tr.train_step(gVTp, uvp, yc, paras, scaler)
        torch.cuda.synchronize()
        res[name + "_layers"] = np.int64(sum(e.dz_coef is not None for e in tr.model_uvp.engine().convs))
        res[name + "_eager_grad"] = tr.flat.grad.cpu().numpy()
        res[name + "_eager_param"] = tr.flat.param.cpu().numpy()
        tg = trainer(True)
        tg.train_step(gVTp, uvp, yc, paras, scaler)            # warm-up, capture, one replay, Adam
        torch.cuda.synchronize()
        res[name + "_graph_grad"] = tg.flat.grad.cpu().numpy()
        res[name + "_graph_param"] = tg.flat.param.cpu().numpy()
        for k in ("1", "2"):                                   # the captured chain alone, twice, on unchanged parameters
            tg._graph.replay()
            torch.cuda.synchronize()
            res[name + "_replay" + k] = tg.flat.grad.cpu().numpy()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])

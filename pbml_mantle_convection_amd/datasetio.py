"""Datasets of the Stokes-surrogate trainer with the reference's item layouts (reference
datasetio.py) plus the seeded synthetic generator used where the /plp_scr1 data files are
absent.

  ADTimeDataset.__getitem__  -> (x[10,H,W], y[3,H,W], scaler, paras[3,1,1], yc[1,H,W])   (:229-280)
  NewADDataset.__getitem__   -> (x[7,H,W], y[2|3,H,W], t_weight, scaler)                 (:595-654)

File loading uses torch.load(weights_only=True): nothing from a data file is executed.
"""
import copy   # noqa: F401  (names the reference exports through its star imports)
import os
import random
import time   # noqa: F401

import numpy as np
import torch
import torch.nn as nn   # noqa: F401
import torch.nn.functional as F   # noqa: F401
from torch.utils.data import DataLoader, Dataset   # noqa: F401

from .pytorch_networks_convae import eta_torch
from .scaler import *   # noqa: F401,F403
from .scaler import velocity_scaler

# normalisation constants of (RaQ, log10 FKT, log10 FKP) (reference :124-136)
RAQ_RANGE = (0.12624371, 9.70723344)
LOG_FKT_RANGE = (6.00352841978384, 9.888820429862925)
LOG_FKP_RANGE = (0.005251646002323797, 1.9927988938926755)
IGNORED_SIMS = (8, 39)


def _load(path):
    return torch.load(path, weights_only=True)


def get_sdf(x, y):
    """Distance to the nearest wall of the box (reference :13-22)."""
    dx = torch.minimum(torch.abs(x - x.min()), torch.abs(x - x.max()))
    dy = torch.minimum(torch.abs(y - y.min()), torch.abs(y - y.max()))
    return torch.minimum(dx, dy)


def eta(gamma, beta, z, T, Tref=0, zref=0):
    return np.exp(np.log(gamma) * (Tref - T) + np.log(beta) * (z - zref))


def normalise_parameters(raq, fkt, fkp):
    return ((raq - RAQ_RANGE[0]) / (RAQ_RANGE[1] - RAQ_RANGE[0]),
            (np.log10(fkt) - LOG_FKT_RANGE[0]) / (LOG_FKT_RANGE[1] - LOG_FKT_RANGE[0]),
            (np.log10(fkp) - LOG_FKP_RANGE[0]) / (LOG_FKP_RANGE[1] - LOG_FKP_RANGE[0]))


def _selected_sims(data_dir, an):
    for si, sim in enumerate(_load(data_dir + "/sims.pt")):
        if sim[1] == an and si not in IGNORED_SIMS:
            yield sim, data_dir + "/" + sim[1] + "/sim_" + str(sim[0])


def get_indices_time(data_dir, an, is_init=False, debug=True, roll_forward=1):
    """(simulation id, time) pairs that have a successor roll_forward steps ahead (reference :30-60)."""
    sims_vec, times_vec = [], []
    for sim, d in _selected_sims(data_dir, "train" if an == "train" else "cv"):
        if debug:
            n = _load(d + "/e1_uprev_data_select_init.pt").repeat(roll_forward * 2, 1, 1, 1).shape[0]
            times = _load(d + "/times.pt")[:n]
        else:
            times = _load(d + "/times.pt")[:750, ...][:-2]
        for i, t in enumerate(times):
            if i < len(times) - roll_forward - 1:
                sims_vec.append(sim[0])
                times_vec.append(t)
    return sims_vec, times_vec


def get_indices(data_dir, an, is_init=False, debug=True, roll_forward=1):
    """(simulation id, snapshot index) pairs of the sub-sampled snapshot files (reference :283-317)."""
    sims_vec, times_vec = [], []
    for sim, d in _selected_sims(data_dir, "train" if an == "train" else "cv"):
        if is_init:
            i_vec = _load(d + "/e1_i_vec_select_init.pt")
        elif debug:
            i_vec = np.arange(_load(d + "/e1_uprev_data_select_snaps.pt").shape[0])
        else:
            i_vec = _load(d + "/e1_i_vec_select.pt")
        for i_prev in i_vec:
            sims_vec.append(sim[0])
            times_vec.append(i_prev)
    return sims_vec, times_vec


class _GridMixin:
    def _load_grid(self, d):
        xc, yc = _load(d + "/xc.pt"), _load(d + "/yc.pt")
        self.xc = xc.view(1, *xc.shape).clone()
        self.yc = yc.view(1, *yc.shape).clone()
        self.xc[:, :, 0], self.xc[:, :, -1] = 0, 4          # wall nodes (reference :158-161, 401-404)
        self.yc[:, 0, :], self.yc[:, -1, :] = 0, 1


class ADTimeDataset(Dataset, _GridMixin):
    """Consecutive-snapshot pairs for the U-Net (reference :63-280)."""

    def __init__(self, data_dir, an, scale=True, load=False, is_init=False, p_pred=True, noise=0.0, debug=True,
                 sims_vec=[], times_vec=[], roll_forward=1):
        self.y_data, self.x_data, self.t_data, self.t = [], [], [], []
        self.paras, self.paras_nd, self.indices, self.indices_init = [], [], [], []
        self.scale, self.p_pred, self.noise = scale, p_pred, noise
        cntr = 0
        tv, sv = np.asarray(times_vec), np.asarray(sims_vec)
        for si, sim in enumerate(_load(data_dir + "/sims.pt")):
            _, _, raq, fkt, fkp, _, _, _ = sim
            d = data_dir + "/" + sim[1] + "/sim_" + str(sim[0])
            wanted = (sim[1] == an) and (len(sims_vec) == 0 or sim[0] in sims_vec)
            times = _load(d + "/times.pt")
            if not (wanted and si not in IGNORED_SIMS and len(times) > 1):
                continue
            nd = normalise_parameters(raq, fkt, fkp)
            self._load_grid(d)
            paras = torch.tensor([raq, fkt, fkp], dtype=torch.float64).view(3, 1, 1)
            paras_nd = torch.tensor(nd, dtype=torch.float64).view(3, 1, 1)
            if debug:
                if p_pred:
                    raise ValueError("p_pred is not implemented in debug mode")
                reps = max(1, int(roll_forward / 2 * 2))
                u, v, Tp = (_load(d + f"/e1_{k}prev_data_select_init.pt").repeat(reps, 1, 1, 1) for k in "uvT")
            else:
                u, v, Tp = (_load(d + f"/e1_{k}prev_data.pt")[:760, ...] for k in "uvT")
                if p_pred:
                    p = _load(d + "/e1_pprev_data.pt")[:760, ...]
            times = times[: u.shape[0]]
            mine = tv[sv == sim[0]] if len(sims_vec) > 0 else None
            for i, t in enumerate(times):
                keep = True if mine is None else (t in mine)
                if keep and i < len(times) - roll_forward - 1:
                    self.indices.append([cntr, cntr + roll_forward])
                    if i == 0:
                        self.indices_init.append([cntr, cntr + roll_forward])
                cntr += 1
                self.paras.append(paras)
                self.paras_nd.append(paras_nd)
                self.x_data.append(Tp[i, ...])
                self.y_data.append(torch.cat((u[i], v[i], p[i]) if p_pred else (u[i], v[i]), axis=0))
                self.t_data.append(torch.tensor(t, dtype=torch.float64))
                self.t.append(t)
        self.num_examples = len(self.indices)

    def __len__(self):
        return self.num_examples

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        i0, i1 = self.indices[idx]
        if i0 % 8 == 0:
            i0, i1 = random.choice(self.indices_init)
        par = self.paras[i0]
        assert torch.all(par == self.paras[i1])
        scaler = velocity_scaler(par[0:1], par[1:2], par[2:3])
        Tp, y = self.x_data[i0].double(), self.y_data[i0].double()
        V = eta_torch(par[1:2], par[2:3], 1.0 - self.yc, Tp)
        shape = (1, Tp.shape[-2], Tp.shape[-1])
        nd = self.paras_nd[i0]
        x = torch.cat((self.xc, self.yc,
                       torch.tensor(self.t[i1] - self.t[i0], dtype=torch.float64).expand(shape),
                       nd[0:1].expand(shape), nd[1:2].expand(shape), nd[2:3].expand(shape),
                       torch.log10(torch.clip(V, 1e-8, 1.0)) / 8.0, Tp, y[0:1] / scaler, y[1:2] / scaler), axis=0)
        y1 = self.y_data[i1].double()
        y_new = torch.cat((y1[0:1] / scaler, y1[1:2] / scaler, self.x_data[i1].double()), axis=0)
        return x, y_new, scaler, par, self.yc


class NewADDataset(Dataset, _GridMixin):
    """Sub-sampled snapshots T -> (u, v[, p]) for the FluidNet family (reference :320-654).  Shard files per simulation
    directory `<data_dir>/<an>/sim_<n>/`: `times.pt`, `xc.pt`, `yc.pt`, and either the pre-selected snapshots
    `e1_{u,v,p,T}prev_data_select[_init|_snaps].pt` with their original step indices `e1_i_vec_select[_init].pt`
    (load=False, :475-583) or the full series `e1_{u,v,p,T}prev_data.pt` (load=True, :421-473).  Every item carries the
    time weight 6 / (step + 1)^(1/4).  Pinned against the reference's own class on files in this layout by
    tests/golden/g18_newad_dataset.npz."""

    def __init__(self, data_dir, an, scale=True, load=False, is_init=False, p_pred=True, noise=0.0, debug=True,
                 sims_vec=[], times_vec=[], max_examples_percent_per_epoch=100):
        self.y_data, self.x_data, self.t_data, self.paras, self.paras_nd = [], [], [], [], []
        self.scale, self.p_pred, self.noise = scale, p_pred, noise
        tv, sv = np.asarray(times_vec), np.asarray(sims_vec)

        def add(i, step, u, v, p, Tp, paras, paras_nd):
            self.paras.append(paras)
            self.paras_nd.append(paras_nd)
            self.x_data.append(Tp[i])
            self.y_data.append(torch.cat((u[i], v[i], p[i]) if p_pred else (u[i], v[i]), axis=0))
            # (`step` is an element of the loaded index tensor: integer-tensor ** 0.25 is evaluated in float32 by torch, and
            # that float32 value is what the reference stores -- the same expression on the same type reproduces it)
            self.t_data.append(torch.as_tensor(6 / (step + 1) ** 0.25).to(torch.float64).reshape(()))

        for si, sim in enumerate(_load(data_dir + "/sims.pt")):
            _, _, raq, fkt, fkp, _, _, _ = sim
            d = data_dir + "/" + sim[1] + "/sim_" + str(sim[0])
            wanted = (sim[1] == an) and (len(sims_vec) == 0 or sim[0] in sims_vec)
            times = _load(d + "/times.pt")
            if not (wanted and si not in IGNORED_SIMS and len(times) > 1):
                continue
            self._load_grid(d)
            paras = torch.tensor([raq, fkt, fkp], dtype=torch.float64).view(3, 1, 1)
            paras_nd = torch.tensor(normalise_parameters(raq, fkt, fkp), dtype=torch.float64).view(3, 1, 1)
            if load:
                # full series, sub-sampled here: the first 200 steps and up to 500 random later ones (:421-473)
                from .scaler import scale_var
                u, v = _load(d + "/e1_uprev_data.pt"), _load(d + "/e1_vprev_data.pt")
                if scale:
                    u, v = scale_var(u, raq, fkt, fkp, "uprev"), scale_var(v, raq, fkt, fkp, "vprev")
                p = _load(d + "/e1_pprev_data.pt") if p_pred else None
                Tp = _load(d + "/e1_Tprev_data.pt")
                nt = len(times) - 2
                if nt > 700:
                    rest = list(range(200, nt))
                    steps = list(range(1, 200)) + random.choices(rest, k=min(500, rest[-1] - 200))
                else:
                    steps = list(range(1, nt))
                steps = steps[:5] if is_init else steps[5:]
                if debug:
                    steps = steps[-8:]
                for i in steps:
                    add(i, i, u, v, p, Tp, paras, paras_nd)
                continue
            if is_init:
                suffix = "_select_init"
            elif debug:
                if p_pred:
                    raise ValueError("p_pred is not implemented in debug mode")
                suffix = "_select_snaps"
            else:
                suffix = "_select"
            u, v, Tp = (_load(d + f"/e1_{k}prev_data{suffix}.pt") for k in "uvT")
            p = _load(d + f"/e1_pprev_data{suffix}.pt") if p_pred else None
            i_vec = np.arange(u.shape[0]) if suffix == "_select_snaps" else _load(d + f"/e1_i_vec{suffix}.pt")
            mine = tv[sv == sim[0]] if len(sims_vec) > 0 else None
            for i, step in enumerate(i_vec):
                if mine is None or step in mine:
                    add(i, step, u, v, p, Tp, paras, paras_nd)
        self.num_examples = min(int(len(self.y_data) * max_examples_percent_per_epoch / 100), len(self.y_data))
        print("using ", self.num_examples, " out of ", len(self.y_data), " per epoch")

    def __len__(self):
        return self.num_examples

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        par, nd = self.paras[idx], self.paras_nd[idx]
        Tp = self.x_data[idx].double().clone()
        if self.noise > 0:
            n = torch.tensor(np.random.uniform(-1e-5, 1e-5, size=(1, Tp.shape[-2] - 4, Tp.shape[-1] - 4)))
            Tp[:, 2:-2, 2:-2] = torch.clip(Tp[:, 2:-2, 2:-2] + n, 0.0, 1.35)
        y = self.y_data[idx].double()
        V = torch.clip(eta_torch(par[1:2], par[2:3], 1.0 - self.yc, Tp), 1e-08, 1)
        if not self.scale:
            raise NotImplementedError("scale=False returns nothing in the reference either")
        scaler = velocity_scaler(par[0:1], par[1:2], par[2:3])
        shape = (1, Tp.shape[-2], Tp.shape[-1])
        x = torch.cat((self.xc / 4, self.yc / 4, torch.log10(V) / 8, nd[0:1].expand(shape), nd[1:2].expand(shape),
                       nd[2:3].expand(shape), Tp), axis=0)
        parts = (y[0:1] / scaler, y[1:2] / scaler) + ((y[2:3],) if self.p_pred else ())
        return x, torch.cat(parts, axis=0), self.t_data[idx].double(), scaler


# --------------------------------------------------------------------------------------------------
# synthetic mantle fields: same item layout as ADTimeDataset, no files needed
# --------------------------------------------------------------------------------------------------
class ResidentADTimeDataset:
    """an `ADTimeDataset` kept resident in HBM with batches assembled ON the device
    (`mc_assemble_adtime_batch`) — the reference builds every item on the host in fp64 and ships it over PCIe
    (datasetio.py:229-280).  The fields are stored once as f32 ([M,H,W] temperatures, [M,cy,H,W] velocities / pressure,
    [M] times, [M,3] parameters); `assemble(idx)` returns device tensors (x [B,10,H,W], y [B,3,H,W], scaler [B],
    paras [B,3,1,1], yc [1,H,W]) and can write straight into `Trainer.input_buffers()`.

    The item logic is the reference's: pair (i0, i1) = indices[idx], replaced by a random initial-condition pair when
    i0 % 8 == 0 (:236-237; host-side, uses `random` like the reference)."""

    def __init__(self, ds: "ADTimeDataset", device):
        from . import _lib as L
        self._L = L
        L.load()
        dev = torch.device(device)
        f = dict(dtype=torch.float32, device=dev)
        self.T = torch.stack([t.reshape(t.shape[-2], t.shape[-1]) for t in ds.x_data]).to(**f).contiguous()
        self.uv = torch.stack(list(ds.y_data)).to(**f).contiguous()
        self.t = torch.tensor([float(v) for v in ds.t], **f)
        self.paras = torch.stack([p.reshape(3) for p in ds.paras]).to(**f).contiguous()
        self.paras_nd = torch.stack([p.reshape(3) for p in ds.paras_nd]).to(**f).contiguous()
        self.xc = ds.xc.reshape(ds.xc.shape[-2], ds.xc.shape[-1]).to(**f).contiguous()
        self.yc = ds.yc.reshape(ds.yc.shape[-2], ds.yc.shape[-1]).to(**f).contiguous()
        self.indices, self.indices_init = list(ds.indices), list(ds.indices_init)
        self.M, self.cy, self.H, self.W = self.T.shape[0], self.uv.shape[1], self.T.shape[1], self.T.shape[2]
        self.device = dev
        print(f"resident ADTimeDataset: {self.M} snapshots, {_resident_bytes(self)} bytes on {dev}")

    def __len__(self):
        return len(self.indices)

    def store(self):
        """The arrays as an `mc_item_store` (the tensors stay owned by this object)."""
        return _item_store(self, self.uv)

    def pairs(self, idx):
        out = []
        for i in idx:
            i0, i1 = self.indices[int(i)]
            if i0 % 8 == 0 and self.indices_init:
                i0, i1 = random.choice(self.indices_init)
            out.append((i0, i1))
        return out

    def assemble(self, idx, out=None, pairs=None):
        """idx: iterable of dataset indices (or explicit `pairs`).  out: optional dict with preallocated 'gVTp' [B,10,H,W],
        'uvp' [B,3,H,W], 'scaler' [B], 'paras' [B,3] f32 device tensors (e.g. Trainer.input_buffers())."""
        L = self._L
        pr = pairs if pairs is not None else self.pairs(idx)
        B = len(pr)
        ptab = torch.tensor(pr, dtype=torch.int32).to(self.device, non_blocking=True)
        f = dict(dtype=torch.float32, device=self.device)
        o = out or {}
        x = o.get("gVTp") if o.get("gVTp") is not None else torch.empty((B, 10, self.H, self.W), **f)
        y = o.get("uvp") if o.get("uvp") is not None else torch.empty((B, 3, self.H, self.W), **f)
        sc = o.get("scaler") if o.get("scaler") is not None else torch.empty((B,), **f)
        pa = o.get("paras") if o.get("paras") is not None else torch.empty((B, 3), **f)
        if tuple(x.shape) != (B, 10, self.H, self.W) or tuple(y.shape) != (B, 3, self.H, self.W) or sc.numel() != B \
                or pa.numel() != 3 * B:
            raise ValueError("output buffers do not match the batch shape")
        L.call("mc_assemble_adtime_batch", L.ptr(self.T), L.ptr(self.uv), L.ptr(self.t), L.ptr(self.paras),
               L.ptr(self.paras_nd), L.ptr(self.xc), L.ptr(self.yc), L.ptr(ptab), B, self.M, self.cy, self.H, self.W,
               L.ptr(x), L.ptr(y), L.ptr(sc), L.ptr(pa), L.stream())
        return x, y, sc, pa.view(B, 3, 1, 1) if pa.dim() == 2 else pa, self.yc.view(1, self.H, self.W)


class ResidentNewADDataset:
    """SURVEY 8(f) N2 for the FluidNet family: a `NewADDataset` kept resident in HBM, batches assembled ON the device by
    `mc_assemble_newad_batch` (the reference builds every item on the host in fp64: datasetio.py:595-654).  Stored once as
    f32: T [M,H,W], targets [M,cy,H,W] (u, v[, p]), time weights [M], parameters [M,3] (+ normalised), xc / yc [H,W].
    `assemble(idx)` returns device tensors (x [B,7,H,W], y [B,cy,H,W], t_weight [B], scaler [B]) — the 4-tuple of
    `NewADDataset.__getitem__`, batched — and can write x, y straight into `Trainer.input_buffers()`.

    A dataset built with `noise > 0` switches the reference's input noise on (:604-613: U(-1e-5, 1e-5) on the interior of T
    whatever the value, clipped to [0, 1.35]).  It is drawn on the device as a pure function of (`noise_seed`, draw, item,
    pixel) (`mc_newad_noise_host` is the host twin); `assemble` takes the draw from an internal counter unless `draw` is given.
    `is_init` marks the initial-condition store of a `ResidentLoader` (its items draw other noise than the main store's)."""

    def __init__(self, ds: "NewADDataset", device, is_init=False, noise_seed=0):
        from . import _lib as L
        self._L = L
        L.load()
        if not ds.scale:
            raise NotImplementedError("scale=False returns nothing in the reference either")
        dev = torch.device(device)
        f = dict(dtype=torch.float32, device=dev)
        n = ds.num_examples
        self.T = torch.stack([t.reshape(t.shape[-2], t.shape[-1]) for t in ds.x_data[:n]]).to(**f).contiguous()
        self.uvp = torch.stack(list(ds.y_data[:n])).to(**f).contiguous()
        self.t = torch.tensor([float(v) for v in ds.t_data[:n]], **f)
        self.paras = torch.stack([p.reshape(3) for p in ds.paras[:n]]).to(**f).contiguous()
        self.paras_nd = torch.stack([p.reshape(3) for p in ds.paras_nd[:n]]).to(**f).contiguous()
        self.xc = ds.xc.reshape(ds.xc.shape[-2], ds.xc.shape[-1]).to(**f).contiguous()
        self.yc = ds.yc.reshape(ds.yc.shape[-2], ds.yc.shape[-1]).to(**f).contiguous()
        self.M, self.cy, self.H, self.W = self.T.shape[0], self.uvp.shape[1], self.T.shape[1], self.T.shape[2]
        self.p_pred, self.device = ds.p_pred, dev
        self.noise = getattr(ds, "noise", 0.0) > 0
        self.is_init, self.noise_seed, self.draw = bool(is_init), int(noise_seed), 0
        print(f"resident NewADDataset: {self.M} items, {_resident_bytes(self)} bytes on {dev}")

    def __len__(self):
        return self.M

    def store(self):
        """The arrays as an `mc_item_store` (the tensors stay owned by this object)."""
        return _item_store(self, self.uvp)

    def assemble(self, idx, out=None, draw=None):
        """idx: iterable of item indices.  out: optional dict with preallocated 'gVTp' [B,7,H,W] and 'uvp' [B,cy,H,W] f32
        device tensors (e.g. Trainer.input_buffers()).  draw: the noise draw (default: the internal counter, which then
        advances by one)."""
        L = self._L
        idx = [int(i) for i in idx]
        if not idx or min(idx) < 0 or max(idx) >= self.M:
            raise IndexError("item index out of range")
        B = len(idx)
        f = dict(dtype=torch.float32, device=self.device)
        o = out or {}
        x = o.get("gVTp") if o.get("gVTp") is not None else torch.empty((B, 7, self.H, self.W), **f)
        y = o.get("uvp") if o.get("uvp") is not None else torch.empty((B, self.cy, self.H, self.W), **f)
        if tuple(x.shape) != (B, 7, self.H, self.W) or tuple(y.shape) != (B, self.cy, self.H, self.W):
            raise ValueError("output buffers do not match the batch shape")
        tw, sc = torch.empty((B,), **f), torch.empty((B,), **f)
        if self.noise:
            # a one-row epoch table through the step kernel (the batch entry point has no noise arguments)
            if draw is None:
                draw, self.draw = self.draw, self.draw + 1
            itab = torch.tensor([-(i + 1) for i in idx] if self.is_init else idx, dtype=torch.int32).to(self.device)
            cursor = torch.from_numpy(np.array([0, 1, int(draw) & 0xFFFFFFFF, 0], dtype=np.uint32).view(np.int32)).to(self.device)
            st = self.store()
            import ctypes as C
            L.call("mc_assemble_newad_step", C.byref(st), C.byref(st) if self.is_init else None, L.ptr(itab), L.ptr(cursor), 1, B,
                   self.cy, self.H, self.W, 1, self.noise_seed & 0xFFFFFFFF, (self.noise_seed >> 32) & 0xFFFFFFFF, L.ptr(x),
                   L.ptr(y), L.ptr(tw), L.ptr(sc), L.stream())
            return x, y, tw, sc
        itab = torch.tensor(idx, dtype=torch.int32).to(self.device, non_blocking=True)
        L.call("mc_assemble_newad_batch", L.ptr(self.T), L.ptr(self.uvp), L.ptr(self.t), L.ptr(self.paras), L.ptr(self.paras_nd),
               L.ptr(self.xc), L.ptr(self.yc), L.ptr(itab), B, self.M, self.cy, self.H, self.W, L.ptr(x), L.ptr(y), L.ptr(tw),
               L.ptr(sc), L.stream())
        return x, y, tw, sc


def _resident_bytes(res):
    return sum(t.numel() * t.element_size() for t in vars(res).values() if isinstance(t, torch.Tensor))


def _item_store(res, uv):
    L = res._L
    return L.ItemStore(L.ptr(res.T), L.ptr(uv), L.ptr(res.t), L.ptr(res.paras), L.ptr(res.paras_nd), L.ptr(res.xc), L.ptr(res.yc),
                       res.M)


# --------------------------------------------------------------------------------------------------
# resident epoch loop: one epoch's batches as a device table, assembled inside the (captured) step
# --------------------------------------------------------------------------------------------------
def loader_seed(seed: int, rank: int = 0) -> int:
    """64-bit noise seed of a rank's loader: low word seed + rank (ranks draw different noise), high word a fixed tag."""
    return (0x4C4F4144 << 32) | ((int(seed) + int(rank)) & 0xFFFFFFFF)


def epoch_steps(shard_sizes, batch_size, small_batch=0):
    """Steps per epoch: the minimum over the ranks' shards of items // (batch_size - small_batch) -- shards differ by up to
    one item, and ranks that ran different step counts would hang the all-reduce."""
    bm = int(batch_size) - int(small_batch)
    if bm <= 0:
        raise ValueError(f"batch_size {batch_size} leaves no room for main items beside small_batch {small_batch}")
    return min(int(n) // bm for n in shard_sizes)


def epoch_table(n_main, batch_size, small_batch=0, n_init=0, *, seed=0, epoch=0, rank=0, steps=None, pairs=None,
                pairs_init=None):
    """One epoch's batches as an int32 table [steps, B] (host, pure): drawn from a torch.Generator seeded with (seed, epoch,
    rank).  Main items are the dataset in shuffled order in rows of B - small_batch, the last short row dropped
    (prepare_dataloader's drop_last=True); every row gets small_batch items of the init set, distinct within the row (what the
    reference's next(iter(loader_init)) yields, multigpu.py:353-357), stored as -(i + 1); then every row is permuted as a
    whole (:358-360).  With `pairs` (ADTimeDataset.indices) the table is [steps, B, 2]: entry i becomes pairs[i], replaced by
    a random pair of `pairs_init` when its first index is a multiple of 8 (datasetio.py:236-237) -- those draws come last, so
    the index table of the same (seed, epoch, rank) is what the pairs were looked up from."""
    B, sb = int(batch_size), int(small_batch)
    bm = B - sb
    if sb < 0 or bm <= 0:
        raise ValueError(f"batch_size {B} / small_batch {sb}: need 0 <= small_batch < batch_size")
    if sb > n_init:
        raise ValueError(f"small_batch {sb} needs at least as many init items, the init set has {n_init}")
    if pairs is not None and sb:
        raise ValueError("the ADTime table takes its initial-condition pairs from the dataset itself: small_batch must be 0")
    g = torch.Generator(device="cpu")
    g.manual_seed(((int(seed) & 0xFFFFFFFF) << 31) ^ ((int(epoch) & 0xFFFFF) << 11) ^ (int(rank) & 0x7FF))
    most = int(n_main) // bm
    steps = most if steps is None else int(steps)
    if steps > most:
        raise ValueError(f"{steps} steps of {bm} main items need more than the {n_main} items of the dataset")
    tab = torch.randperm(int(n_main), generator=g)[: steps * bm].view(steps, bm)
    if sb and steps:
        init = torch.stack([torch.randperm(int(n_init), generator=g)[:sb] for _ in range(steps)]).view(steps, sb)
        tab = torch.cat((tab, -(init + 1)), dim=1)
        order = torch.stack([torch.randperm(B, generator=g) for _ in range(steps)]).view(steps, B)
        tab = torch.gather(tab, 1, order)
    if pairs is None:
        return tab.to(torch.int32).contiguous()
    pr = torch.tensor(pairs, dtype=torch.int64).view(-1, 2)[tab]                 # [steps, B, 2]
    if pairs_init is not None and len(pairs_init):
        pi = torch.tensor(pairs_init, dtype=torch.int64).view(-1, 2)
        pick = torch.randint(0, pi.shape[0], (steps, B), generator=g)
        pr = torch.where((pr[..., :1] % 8 == 0), pi[pick], pr)
    return pr.to(torch.int32).contiguous()


def validate_table(tab, m_main, m_init=0):
    """Every entry of an epoch table against the store sizes (host, before upload): e >= 0 needs e < m_main, e < 0 needs
    -e - 1 < m_init; the two entries of a pair come from the same store."""
    t = tab.to(torch.int64)
    if t.numel() == 0:
        return
    if int(t.max()) >= int(m_main) or int(t.min()) < -int(m_init):
        raise IndexError(f"epoch table entry outside its store: range [{int(t.min())}, {int(t.max())}] for {m_main} main and "
                         f"{m_init} init items")
    if t.dim() == 3 and bool(((t[..., 0] < 0) != (t[..., 1] < 0)).any()):
        raise IndexError("epoch table pair with entries from two stores")


class ResidentLoader:
    """Iterable over one epoch's batches of a resident dataset (and, for the FluidNet family, a resident initial-condition set:
    `small_batch` of its items go into every batch, reference multigpu.py:353-361, 866-884).  `start_epoch(epoch)` uploads the
    epoch's table (`epoch_table`) into one fixed device buffer; `next_batch()` launches the assembly of the row the device
    cursor points at and the cursor's advance on the current stream.  Table, cursor and output tensors never move, so a captured
    step that contains `launch()` consumes one row per replay (Trainer, use_graph=True).  len() = steps per epoch, the
    minimum over `shard_sizes` (the ranks' item counts; default: this rank's alone)."""

    def __init__(self, resident, resident_init=None, batch_size=None, small_batch=0, seed=0, rank=0, world=1, shard_sizes=None):
        from . import _lib as L
        self._L = L
        self.res, self.res_init = resident, resident_init
        self.adtime = isinstance(resident, ResidentADTimeDataset)
        if resident_init is None:
            small_batch = 0
        elif self.adtime:
            raise ValueError("the ADTime dataset holds its own initial-condition pairs: resident_init must be None")
        elif (resident_init.H, resident_init.W, resident_init.cy) != (resident.H, resident.W, resident.cy):
            raise ValueError("the init set has another grid or target count than the main set")
        if batch_size is None:
            raise ValueError("batch_size is required")
        self.B, self.small_batch, self.seed, self.rank, self.world = int(batch_size), int(small_batch), int(seed), int(rank), int(world)
        self.n_main = len(resident)
        self.n_init = len(resident_init) if self.small_batch else 0
        self.steps = epoch_steps(shard_sizes if shard_sizes is not None else [self.n_main], self.B, self.small_batch)
        if self.steps * (self.B - self.small_batch) > self.n_main:
            raise ValueError("shard_sizes promise more items than the resident dataset holds")
        dev = self.device = resident.device
        self.noise = bool(getattr(resident, "noise", False))
        self.seed64 = loader_seed(seed, rank)
        if not self.adtime:
            resident.noise_seed = self.seed64
            if resident_init is not None:
                resident_init.noise_seed, resident_init.is_init = self.seed64, True
        self._store = resident.store()
        self._store_init = resident_init.store() if self.small_batch else None
        rows = max(self.steps, 1)
        self.rows = rows
        self.table = torch.zeros((rows, self.B, 2) if self.adtime else (rows, self.B), dtype=torch.int32, device=dev)
        self.table_host = self.table.cpu()
        self.cursor = torch.zeros(4, dtype=torch.int32, device=dev)
        self.set_cursor(0, 0)
        f = dict(dtype=torch.float32, device=dev)
        H, W = resident.H, resident.W
        if self.adtime:
            self.out = dict(gVTp=torch.zeros((self.B, 10, H, W), **f), uvp=torch.zeros((self.B, 3, H, W), **f),
                            scaler=torch.zeros((self.B,), **f), paras=torch.zeros((self.B, 3), **f))
        else:
            self.out = dict(gVTp=torch.zeros((self.B, 7, H, W), **f), uvp=torch.zeros((self.B, resident.cy, H, W), **f),
                            scaler=torch.zeros((self.B,), **f), t_weight=torch.zeros((self.B,), **f))
        self.epoch = None

    def __len__(self):
        return self.steps

    def build_table(self, epoch):
        if self.adtime:
            return epoch_table(self.n_main, self.B, seed=self.seed, epoch=epoch, rank=self.rank, steps=self.steps,
                               pairs=self.res.indices, pairs_init=self.res.indices_init)
        return epoch_table(self.n_main, self.B, self.small_batch, self.n_init, seed=self.seed, epoch=epoch, rank=self.rank,
                           steps=self.steps)

    def set_cursor(self, step, draw):
        """cursor = (step, steps, draw, 0) from the host (one small copy on the current stream)."""
        host = np.array([int(step), self.steps, int(draw) & 0xFFFFFFFF, 0], dtype=np.uint32)
        self.cursor.copy_(torch.from_numpy(host.view(np.int32)))

    def cursor_state(self):
        """(step, draw) of the device cursor (host sync; for set-up and tests, never per step)."""
        c = self.cursor.cpu().numpy().view(np.uint32)
        return int(c[0]), int(c[2])

    def _push_noise_seed(self):
        if not self.adtime:
            self.res.noise_seed = self.seed64
            if self.res_init is not None:
                self.res_init.noise_seed = self.seed64

    def state(self):
        """What the next epoch's batches depend on beside the constructor's arguments (plain numbers; one host sync): the table
        seed, the 64-bit noise seed, the datasets' noise_seed and the device cursor.  The epoch's table is a pure function of
        (seed, epoch, rank) and is not part of it."""
        step, draw = self.cursor_state()
        return dict(seed=self.seed, seed64=self.seed64, step=step, draw=draw,
                    noise_seed=[getattr(r, "noise_seed", None) for r in (self.res, self.res_init) if r is not None])

    def load_state(self, st):
        """Restores `state()` in place: the cursor keeps its address (a captured step goes on reading it), and the noise seed
        goes to the resident datasets as in the constructor."""
        self.seed, self.seed64 = int(st["seed"]), int(st["seed64"])
        self._push_noise_seed()
        self.set_cursor(int(st["step"]), int(st["draw"]))

    def start_epoch(self, epoch, table=None):
        """Uploads the epoch's table (one H2D copy into the fixed buffer) and rewinds the cursor's step; the draw goes on."""
        tab = self.build_table(epoch) if table is None else table.to(torch.int32)
        if tuple(tab.shape) != tuple(self.table.shape) and self.steps:
            raise ValueError(f"epoch table of shape {tuple(tab.shape)}, the loader holds {tuple(self.table.shape)}")
        validate_table(tab, self.res.M if self.adtime else self.n_main, self.n_init)
        if self.steps:
            self.table_host = tab
            self.table.copy_(tab)
        self.cursor[0:1].zero_()
        self.epoch = epoch

    def launch(self, out=None):
        """The assembly of the cursor's row into `out` (default: the loader's own fixed tensors) and the cursor's advance, on
        the current stream; capturable."""
        import ctypes as C
        L, o, r = self._L, (out or self.out), self.res
        for k, v in self.out.items():
            if k in o and o[k] is not None and tuple(o[k].shape) != tuple(v.shape):
                raise ValueError(f"output buffer {k!r} of shape {tuple(o[k].shape)}, expected {tuple(v.shape)}")
        g = lambda k: o[k] if o.get(k) is not None else self.out[k]  # noqa: E731
        init = C.byref(self._store_init) if self._store_init is not None else None
        if self.adtime:
            L.call("mc_assemble_adtime_step", C.byref(self._store), init, L.ptr(self.table), L.ptr(self.cursor), self.rows, self.B,
                   r.cy, r.H, r.W, L.ptr(g("gVTp")), L.ptr(g("uvp")), L.ptr(g("scaler")), L.ptr(g("paras")), L.stream())
        else:
            L.call("mc_assemble_newad_step", C.byref(self._store), init, L.ptr(self.table), L.ptr(self.cursor), self.rows, self.B,
                   r.cy, r.H, r.W, int(self.noise), self.seed64 & 0xFFFFFFFF, self.seed64 >> 32, L.ptr(g("gVTp")),
                   L.ptr(g("uvp")), L.ptr(g("t_weight")), L.ptr(g("scaler")), L.stream())
        L.call("mc_loader_advance", L.ptr(self.cursor), L.stream())
        return g

    def batch(self, g=None):
        """The output tensors in the item layout of the host datasets (what Trainer._unpack expects)."""
        g = g or (lambda k: self.out[k])
        r = self.res
        if self.adtime:
            return g("gVTp"), g("uvp"), g("scaler"), g("paras").view(self.B, 3, 1, 1), r.yc.view(1, r.H, r.W)
        return g("gVTp"), g("uvp"), g("t_weight"), g("scaler")

    def next_batch(self, out=None):
        """Assembles the next batch on the device (no host copy): the eager form of the loop and the cv form."""
        if self.epoch is None:
            self.start_epoch(0)
        return self.batch(self.launch(out))

    def __iter__(self):
        for _ in range(self.steps):
            yield self.next_batch()


def synthetic_batch(B, H, W, seed, *, p_pred=True, device="cpu", dtype=torch.float32, channels=None):
    """Seeded synthetic (gVTp, uvp, scaler, paras, yc) with the statistics of the real data:
    T = conductive profile + Gaussian plumes; parameters from the dataset's ranges; previous and
    target velocities from random streamfunctions (divergence-free targets); p low-pass random."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    y1 = torch.linspace(0, 1, H, dtype=torch.float64)
    x1 = torch.linspace(0, 4, W, dtype=torch.float64)
    yy, xx = y1[:, None].expand(H, W), x1[None, :].expand(H, W)

    def U(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)

    def stream_uv():
        psi_y = torch.zeros(B, H, W, dtype=torch.float64)
        psi_x = torch.zeros(B, H, W, dtype=torch.float64)
        for _ in range(8):
            a, kx, ky = U(-1, 1, B, 1, 1), U(0.5, 6, B, 1, 1), U(1, 8, B, 1, 1)
            px, py = U(0, 6.28, B, 1, 1), U(0, 6.28, B, 1, 1)
            psi_y = psi_y + a * ky * torch.sin(kx * xx + px) * torch.cos(ky * yy + py)    # d psi / dy
            psi_x = psi_x + a * kx * torch.cos(kx * xx + px) * torch.sin(ky * yy + py)    # d psi / dx
        s = 0.1 / psi_y.abs().mean().clamp_min(1e-9)
        return s * psi_y, -s * psi_x

    def smooth(amp):
        f = torch.zeros(B, H, W, dtype=torch.float64)
        for _ in range(6):
            f = f + U(-1, 1, B, 1, 1) * torch.sin(U(0.5, 5, B, 1, 1) * xx + U(0, 6.28, B, 1, 1)) * \
                torch.cos(U(0.5, 6, B, 1, 1) * yy + U(0, 6.28, B, 1, 1))
        return amp * f / 3.0

    def temperature():
        T = (1.0 - yy).expand(B, H, W).clone()
        for _ in range(4):
            a, s = U(0.05, 0.3, B, 1, 1), U(0.03, 0.15, B, 1, 1)
            cx, cy = U(0, 4, B, 1, 1), U(0, 1, B, 1, 1)
            T = T + a * torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
        T = torch.clip(T + 1e-3 * torch.randn(B, H, W, generator=g, dtype=torch.float64), 0.0, 1.35)
        T[:, 0, :], T[:, -1, :] = 1.0, 0.0
        T[:, :, 0], T[:, :, -1] = T[:, :, 1], T[:, :, -2]
        return T

    raq = U(RAQ_RANGE[0], RAQ_RANGE[1], B)
    fkt = 10.0 ** U(LOG_FKT_RANGE[0], LOG_FKT_RANGE[1], B)
    fkp = 10.0 ** U(LOG_FKP_RANGE[0], LOG_FKP_RANGE[1], B)
    nd = [t.view(B, 1, 1).expand(B, H, W) for t in normalise_parameters(raq, fkt, fkp)]
    T0, T1 = temperature(), temperature()
    u0, v0 = stream_uv()
    u1, v1 = stream_uv()
    p0, p1 = smooth(0.5), smooth(0.5)
    V = torch.log10(torch.clip(eta_torch(fkt.view(B, 1, 1), fkp.view(B, 1, 1), 1.0 - yy, T0), 1e-8, 1.0)) / 8.0
    dt = U(1e-7, 1e-4, B).view(B, 1, 1).expand(B, H, W)
    chans = [xx.expand(B, H, W), yy.expand(B, H, W), dt, nd[0], nd[1], nd[2], V, T0, u0, v0]
    if p_pred:
        chans.append(p0)
    gVTp = torch.stack(chans, 1)
    if channels is not None:
        gVTp = gVTp[:, :channels]
    uvp = torch.stack([u1, v1, p1, T1] if p_pred else [u1, v1, T1], 1)
    scaler = torch.as_tensor(velocity_scaler(raq.numpy(), fkt.numpy(), fkp.numpy()))
    paras = torch.stack([raq, fkt, fkp], 1)
    to = dict(device=device, dtype=dtype)
    return gVTp.to(**to), uvp.to(**to), scaler.to(**to), paras.to(**to), yy.contiguous().to(**to)


class SyntheticMantleDataset(Dataset):
    """ADTimeDataset-shaped items from `synthetic_batch` (generated once, kept in host RAM)."""

    def __init__(self, n, H, W, p_pred=True, seed=1234, network="unet", c_i=None):
        chunk = 8
        parts = [synthetic_batch(min(chunk, n - i), H, W, seed + i, p_pred=p_pred) for i in range(0, n, chunk)]
        self.x = torch.cat([p[0] for p in parts])
        self.y = torch.cat([p[1] for p in parts])
        self.scaler = torch.cat([p[2] for p in parts])
        self.paras = torch.cat([p[3] for p in parts])
        self.yc = parts[0][4]
        self.network = network
        if network == "convae":
            # ConvAE plumbing config (CFG-1): T (+ two parameter maps) -> (u, v, p)
            self.x = torch.stack([self.x[:, 7], self.x[:, 3], self.x[:, 4]], 1) if (c_i or 3) == 3 else self.x[:, :c_i]
            self.y = self.y[:, :3]
        elif "fluidnet" in network:
            # (fluidnet / ifluidnet / newfluidnet, the reference's `"fluidnet" in self.net`) NewADDataset-shaped items of the FluidNet branch: 7 input channels, truth (u, v[, p]) without T
            self.x = self.x[:, :(c_i or 7)]
            self.y = self.y[:, :3] if p_pred else self.y[:, :2]

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        if self.network == "convae" or "fluidnet" in self.network:
            return self.x[i], self.y[i], torch.tensor(0.0), self.scaler[i]
        return self.x[i], self.y[i], self.scaler[i], self.paras[i].view(3, 1, 1), self.yc.view(1, *self.yc.shape)

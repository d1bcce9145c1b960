"""The resident epoch loop on the device: the step kernels (`mc_assemble_newad_step`, `mc_assemble_adtime_step`, indices from
a device epoch table and cursor) against the batch kernels, the input noise against its host twin, a Trainer whose captured
step assembles its own batches against a hand-fed eager Trainer, and a CLI run that never builds a host DataLoader.
Fixtures: the shard trees of g18 (10 x 14) and g19 (8 x 12)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _write_tree(g, root):
    sims = [(int(n), str(a), *[float(v) for v in par[:5]], int(par[5])) for n, a, par in zip(g["sims_num"], g["sims_an"], g["sims_par"])]
    torch.save(sims, os.path.join(root, "sims.pt"))
    for k in g.files:
        if not k.startswith("file/"):
            continue
        _, an, sim, name = k.split("/")
        d = os.path.join(root, an, sim)
        os.makedirs(d, exist_ok=True)
        torch.save(torch.from_numpy(g[k]), os.path.join(d, name + ".pt"))
    return sims


class _Tree(dict):
    """A golden archive as a dict whose arrays a test may change before writing the tree."""
    @property
    def files(self):
        return list(self)


ZERO_AT, HOT_AT = (4, 5), (5, 6)        # interior pixels of every T field set to 0 and to 1.35: both clip sides occur


def _newad(golden, root, noise=0.0, clip_values=False):
    """(train, train init, cv, cv init) NewADDatasets of the g18 tree."""
    from pbml_mantle_convection_amd.datasetio import NewADDataset
    g = _Tree({k: np.array(v) for k, v in golden("g18_newad_dataset").items()})
    if clip_values:
        for k in g:
            if "Tprev_data_select" in k:
                g[k][:, 0, ZERO_AT[0], ZERO_AT[1]] = 0.0
                g[k][:, 0, HOT_AT[0], HOT_AT[1]] = 1.35
    os.makedirs(root, exist_ok=True)
    _write_tree(g, str(root))
    kw = dict(scale=True, load=False, p_pred=True, debug=False, noise=noise)
    return tuple(NewADDataset(str(root), an, is_init=init, **kw) for an in ("train", "cv") for init in (False, True))


def _adtime(golden, root):
    from pbml_mantle_convection_amd.datasetio import ADTimeDataset
    os.makedirs(root, exist_ok=True)
    _write_tree(golden("g19_adtime_dataset"), str(root))
    return tuple(ADTimeDataset(str(root), an, scale=True, load=False, p_pred=False, debug=False, roll_forward=1)
                 for an in ("train", "cv"))


def _banded(shape, band=64):
    """A tensor between two NaN bands of one allocation: (view, whole)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * band,), float("nan"), device=DEV)
    return whole[band:band + n].view(shape), whole


def _bands_intact(whole, n, band=64):
    return bool(torch.isnan(whole[:band]).all()) and bool(torch.isnan(whole[band + n:]).all()) and \
        not bool(torch.isnan(whole[band:band + n]).any())


def test_newad_step_kernel_equals_batch_kernel_row_by_row(golden, tmp_path):
    from pbml_mantle_convection_amd.datasetio import ResidentLoader, ResidentNewADDataset
    ds, ds_init, _, _ = _newad(golden, tmp_path)
    res, res_init = ResidentNewADDataset(ds, DEV), ResidentNewADDataset(ds_init, DEV, is_init=True)
    assert len(res) == 10 and len(res_init) == 6
    ld = ResidentLoader(res, res_init, batch_size=4, small_batch=2, seed=1, shard_sizes=[6])
    assert len(ld) == 3
    table = torch.tensor([[0, -1, 9, -6], [-3, 3, 3, -2], [5, -4, -5, 2]], dtype=torch.int32)
    ld.start_epoch(0, table=table)
    shapes = dict(gVTp=(4, 7, 10, 14), uvp=(4, 3, 10, 14), t_weight=(4,), scaler=(4,))
    for visit in range(4):                                             # rows 0, 1, 2 and the wrap to 0
        row = table[visit % 3].tolist()
        assert ld.cursor_state() == (visit % 3, visit)
        bufs = {k: _banded(s) for k, s in shapes.items()}
        x, y, tw, sc = ld.next_batch({k: v[0] for k, v in bufs.items()})
        torch.cuda.synchronize()
        for k, s in shapes.items():
            assert _bands_intact(bufs[k][1], int(np.prod(s))), k
        for b, e in enumerate(row):
            xr, yr, tr, sr = (res.assemble([e]) if e >= 0 else res_init.assemble([-e - 1]))
            assert torch.equal(x[b], xr[0]) and torch.equal(y[b], yr[0]), (visit, b)
            assert torch.equal(tw[b], tr[0]) and torch.equal(sc[b], sr[0]), (visit, b)
    with pytest.raises(IndexError):
        ld.start_epoch(1, table=torch.tensor([[0, 1, 10, -1]] * 3))     # item 10 of 10
    with pytest.raises(IndexError):
        ld.start_epoch(1, table=torch.tensor([[0, 1, 2, -7]] * 3))      # init item 6 of 6
    # without an init store a negative entry never reaches the device
    ld0 = ResidentLoader(res, None, batch_size=4, seed=1)
    assert len(ld0) == 2 and int(ld0.build_table(0).min()) >= 0
    with pytest.raises(IndexError):
        ld0.start_epoch(0, table=torch.tensor([[0, 1, 2, -1]] * 2))


def test_adtime_step_kernel_equals_batch_kernel_row_by_row(golden, tmp_path):
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd.datasetio import ResidentADTimeDataset, ResidentLoader
    ds, ds_cv = _adtime(golden, tmp_path)
    res, other = ResidentADTimeDataset(ds, DEV), ResidentADTimeDataset(ds_cv, DEV)
    # the kernel itself, with a second store behind the negative entries
    table = torch.tensor([[[1, 2], [-1, -2], [19, 20], [-9, -10]], [[0, 1], [0, 1], [-5, -6], [12, 13]],
                          [[-2, -3], [7, 8], [3, 4], [-1, -2]]], dtype=torch.int32, device=DEV)
    cursor = torch.from_numpy(np.array([0, 3, 0, 0], dtype=np.uint32).view(np.int32)).to(DEV)
    s0, s1 = res.store(), other.store()
    shapes = dict(x=(4, 10, 8, 12), y=(4, 3, 8, 12), sc=(4,), pa=(4, 3))
    for visit in range(4):
        bufs = {k: _banded(s) for k, s in shapes.items()}
        L.call("mc_assemble_adtime_step", C.byref(s0), C.byref(s1), L.ptr(table), L.ptr(cursor), 3, 4, res.cy, 8, 12,
               L.ptr(bufs["x"][0]), L.ptr(bufs["y"][0]), L.ptr(bufs["sc"][0]), L.ptr(bufs["pa"][0]), L.stream())
        L.call("mc_loader_advance", L.ptr(cursor), L.stream())
        torch.cuda.synchronize()
        assert cursor.cpu().numpy().view(np.uint32).tolist() == [(visit + 1) % 3, 3, visit + 1, 0]
        for k, s in shapes.items():
            assert _bands_intact(bufs[k][1], int(np.prod(s))), k
        for b, (e0, e1) in enumerate(table[visit % 3].tolist()):
            xr, yr, sr, pr, _ = res.assemble(None, pairs=[(e0, e1)]) if e0 >= 0 else other.assemble(None, pairs=[(-e0 - 1, -e1 - 1)])
            assert torch.equal(bufs["x"][0][b], xr[0]) and torch.equal(bufs["y"][0][b], yr[0]), (visit, b)
            assert torch.equal(bufs["sc"][0][b], sr[0]) and torch.equal(bufs["pa"][0][b], pr.reshape(3)), (visit, b)
    # the loader: pairs from the dataset, scaler / paras / yc in the layout of the host items
    ld = ResidentLoader(res, None, batch_size=4, seed=2)
    assert len(ld) == 18 // 4
    ld.start_epoch(0)
    init = {tuple(p) for p in ds.indices_init}
    for step in range(len(ld)):
        row = ld.table_host[step].tolist()
        assert all(p[0] % 8 != 0 or tuple(p) in init for p in row)
        x, y, sc, pa, yc = ld.next_batch()
        xr, yr, sr, pr, ycr = res.assemble(None, pairs=[tuple(p) for p in row])
        assert torch.equal(x, xr) and torch.equal(y, yr) and torch.equal(sc, sr) and torch.equal(pa, pr)
        assert tuple(pa.shape) == (4, 3, 1, 1) and tuple(yc.shape) == (1, 8, 12) and torch.equal(yc, ycr)
    assert ld.cursor_state() == (0, len(ld))


def test_noise_equals_the_host_twin_and_leaves_frame_and_targets_alone(golden, tmp_path):
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd.datasetio import ResidentLoader, ResidentNewADDataset
    from pbml_mantle_convection_amd.pytorch_networks_convae import eta_torch
    ds0 = _newad(golden, tmp_path / "clean", noise=0.0, clip_values=True)[0]
    ds1, ds1_init = _newad(golden, tmp_path / "noisy", noise=0.1, clip_values=True)[:2]
    res0, res1 = ResidentNewADDataset(ds0, DEV), ResidentNewADDataset(ds1, DEV)
    res1_init = ResidentNewADDataset(ds1_init, DEV, is_init=True)
    assert not res0.noise and res1.noise
    idx = list(range(len(res1)))
    ld = ResidentLoader(res1, None, batch_size=len(idx), seed=11)
    ld.start_epoch(0, table=torch.tensor([idx], dtype=torch.int32))
    seed = ld.seed64
    x0, y0, t0, s0 = res0.assemble(idx)
    x1, y1, t1, s1 = (t.clone() for t in ld.next_batch())             # draw 0
    x2 = ld.next_batch()[0].clone()                                   # draw 1, the same items
    assert ld.cursor_state() == (0, 2)
    ld.set_cursor(0, 0)
    x3 = ld.next_batch()[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and torch.equal(t1, t0) and torch.equal(s1, s0)
    assert not torch.equal(x2[:, 6], x1[:, 6]) and torch.equal(x3, x1)
    for c in (0, 1, 3, 4, 5):
        assert torch.equal(x1[:, c], x0[:, c])
    lib = L.load()
    H, W = 10, 14

    def expect(T_clean, draw, item_word):
        e = T_clean.copy()
        for r in range(2, H - 2):
            for c in range(2, W - 2):
                n = np.float32(lib.mc_newad_noise_host(seed & 0xFFFFFFFF, seed >> 32, draw, item_word, r * W + c))
                e[r, c] = np.float32(T_clean[r, c] + n)
        return e

    low = high = 0
    Tc, Tn = x0[:, 6].cpu().numpy(), x1[:, 6].cpu().numpy()
    hot = np.float32(1.35)
    for b, i in enumerate(idx):
        d = Tn[b] - Tc[b]
        frame = np.ones((H, W), bool)
        frame[2:-2, 2:-2] = False
        assert np.all(d[frame] == 0.0)                                  # the two-pixel frame: untouched and unclipped
        raw = expect(Tc[b], 0, i)
        inside = (raw >= 0) & (raw <= hot)
        assert np.array_equal(Tn[b][inside], raw[inside])               # bit for bit where T + n stays inside [0, 1.35]
        assert np.all(Tn[b][raw < 0] == 0.0) and np.all(Tn[b][raw > hot] == hot)
        low, high = low + int((raw < 0).sum()), high + int((raw > hot).sum())
        assert np.all(np.abs(d) <= 1e-5 + 1.2e-7)                       # |n| < 1e-5 and half an ulp of a sum below 2
        raw2 = expect(Tc[b], 1, i)                                      # the next draw
        inside2 = (raw2 >= 0) & (raw2 <= hot)
        assert np.array_equal(x2[b, 6].cpu().numpy()[inside2], raw2[inside2])
    assert low > 0 and high > 0, (low, high)
    # the viscosity channel follows the noisy T (f64 restatement, the tolerance of test_dataset_shards.py for this channel)
    for b, i in enumerate(idx):
        par = ds1.paras[i]
        V = torch.clip(eta_torch(par[1:2], par[2:3], 1.0 - ds1.yc, torch.from_numpy(Tn[b]).double().view(1, H, W)), 1e-8, 1)
        np.testing.assert_allclose(x1[b, 2].cpu().numpy(), (torch.log10(V) / 8)[0].numpy(), rtol=2e-5, atol=2e-6)
    assert not torch.equal(x1[:, 2], x0[:, 2])
    # assemble(): the same noise from its own draw counter, whatever the batch position; the init store draws other noise
    xa = res1.assemble(idx)[0]
    xb = res1.assemble(idx)[0]
    assert (res1.draw, torch.equal(xa, x1), torch.equal(xb, x2)) == (2, True, True)
    assert torch.equal(res1.assemble(idx[::-1], draw=0)[0].flip(0), x1)
    assert torch.equal(res1.assemble([3], draw=1)[0][0], x2[3])
    ld_i = ResidentLoader(res1, res1_init, batch_size=3, small_batch=2, seed=11)
    ld_i.start_epoch(0, table=torch.tensor([[2, -3, -1]] * len(ld_i), dtype=torch.int32))
    xi = ld_i.next_batch()[0].clone()
    assert torch.equal(xi[0], x1[2]) and torch.equal(xi[1], res1_init.assemble([2], draw=0)[0][0])
    Ti = res1_init.T[2].cpu().numpy()
    assert np.array_equal(xi[1, 6].cpu().numpy()[3, 3:6], expect(Ti, 0, 2 | 0x80000000)[3, 3:6])
    assert not np.array_equal(expect(Ti, 0, 2 | 0x80000000)[3, 3:6], expect(Ti, 0, 2)[3, 3:6])


def _trainer(model, network, use_graph, precision, train=None, cv=None, lambda_mom=0.0, p_pred=True):
    from pbml_mantle_convection_amd.multigpu import Trainer
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.5)
    return Trainer(model, None, train, cv, None, None, opt, sch, 0, 1, "/tmp/", p_pred=p_pred, network=network, loss_scale=True,
                   loss_type="mass", precision=precision, use_graph=use_graph, lambda_mom=lambda_mom, drop_seed=0)


def _hand_newad(res, res_init, row, draw):
    parts = [(res.assemble([e], draw=draw) if e >= 0 else res_init.assemble([-e - 1], draw=draw)) for e in row]
    x, y = (torch.cat([p[k] for p in parts]) for k in range(2))
    return x, y, None, None, None                                      # (the FluidNet family's loss takes no scaler)


def _hand_adtime(res, _none, row, draw):
    x, y, sc, pa, yc = res.assemble(None, pairs=[tuple(p) for p in row])
    return x, y, yc, pa, sc


def _same_state(a, b, tag):
    torch.cuda.synchronize()
    for name in ("param", "grad"):
        assert torch.equal(getattr(a.flat, name), getattr(b.flat, name)), (tag, name)
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq), tag


@pytest.mark.parametrize("precision", ["fp32", "mixed"])
@pytest.mark.parametrize("net", ["newfluidnet", "unet"])
def test_captured_resident_steps_equal_hand_fed_eager_steps(golden, tmp_path, net, precision):
    """Trainer A: ResidentLoaders, use_graph=True (the replay assembles the batch).  Trainer B: the same weights, fed with
    `assemble` of the same table rows and draws, eager.  Two epochs (a table refresh in between): parameters and both Adam
    moments stay bit-identical after every step, and so do the cv losses."""
    from pbml_mantle_convection_amd.datasetio import ResidentADTimeDataset, ResidentLoader, ResidentNewADDataset
    from pbml_mantle_convection_amd.multigpu import build_model
    from pbml_mantle_convection_amd.pytorch_networks_convae import Unet
    if net == "newfluidnet":
        dss = _newad(golden, tmp_path, noise=0.1)
        tr_res, tr_init, cv_res, cv_init = (ResidentNewADDataset(d, DEV, is_init=bool(k % 2)) for k, d in enumerate(dss))
        loaders = [ResidentLoader(tr_res, tr_init, batch_size=4, small_batch=2, seed=3),
                   ResidentLoader(cv_res, cv_init, batch_size=4, small_batch=2, seed=3)]
        assert [len(ld) for ld in loaders] == [5, 2] and loaders[0].noise
        stores, hand, kw = [(tr_res, tr_init), (cv_res, cv_init)], _hand_newad, dict()

        def model():
            torch.manual_seed(4)
            return build_model("newfluidnet", 2, 7, 8, 3, torch.device(DEV), "gelu", "zeros", "mass", True, 1, 3, p_pred=True)
    else:
        tr_res, cv_res = (ResidentADTimeDataset(d, DEV) for d in _adtime(golden, tmp_path))
        loaders = [ResidentLoader(tr_res, None, batch_size=4, seed=3), ResidentLoader(cv_res, None, batch_size=4, seed=3)]
        assert [len(ld) for ld in loaders] == [4, 2]
        stores, hand, kw = [(tr_res, None), (cv_res, None)], _hand_adtime, dict(lambda_mom=1e-6, p_pred=False)

        def model():
            torch.manual_seed(4)
            return Unet(2, 10, 8, 3, torch.device(DEV), "gelu", "reflect", "mass", use_symm=True, repeats=1, f=3, p_pred=False)
    A = _trainer(model(), net, True, precision, loaders[0], loaders[1], **kw)
    B = _trainer(model(), net, False, precision, **kw)
    assert torch.equal(A.flat.param, B.flat.param)
    draws = [0, 0]
    tables = []
    for epoch in range(2):
        for which, ld in enumerate(loaders):
            ld.start_epoch(epoch)
            tables.append(ld.table_host.clone())
            for step in range(len(ld)):
                row = ld.table_host[step].tolist()
                batch = hand(*stores[which], row, draws[which])
                draws[which] += 1
                if which == 0:
                    la, lb = A.resident_step(ld, True).clone(), B.train_step(*batch).clone()
                    _same_state(A, B, (epoch, step))
                else:
                    with torch.no_grad():
                        la, lb = A.resident_step(ld, False).clone(), B.eval_step(*batch).clone()
                assert torch.equal(la, lb) and bool(torch.isfinite(la).all()), (epoch, which, step, la, lb)
            assert ld.cursor_state() == (0, draws[which])              # wrapped; the warm-up pass consumed nothing
    assert not torch.equal(tables[0], tables[2]) and A._graph is not None and B._graph is None
    st = A.input_buffers()
    assert st["gVTp"].data_ptr() == loaders[0].out["gVTp"].data_ptr()   # the captured step reads what the loader writes


def test_cli_resident_run_never_builds_a_host_loader(golden, tmp_path, monkeypatch):
    import torch.distributed as dist
    from pbml_mantle_convection_amd import multigpu as G
    os.makedirs(tmp_path / "data")
    _write_tree(golden("g18_newad_dataset"), str(tmp_path / "data"))

    def no_loader(self, *a, **k):
        raise AssertionError("a host DataLoader was built in a --resident 1 run")

    monkeypatch.setattr(torch.utils.data.DataLoader, "__init__", no_loader)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    try:
        G.cli(["-net", "newfluidnet", "-l", "2", "-f", "8", "-r", "1", "-k", "3", "-p", "zeros", "-lt", "mass", "-pp", "1", "-s", "1",
               "-ab", "10", "-b", "4", "-deb", "0", "-n", "0.1", "--data_dir", str(tmp_path / "data"),
               "--nn_root", str(tmp_path / "nn"), "--precision", "fp32", "--resident", "1", "--use_graph", "1", "--epochs", "2"])
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    runs = os.listdir(tmp_path / "nn")
    assert len(runs) == 1
    d = tmp_path / "nn" / runs[0]
    lines = open(d / "fluidnet_uvpT.txt").read().strip().split("\n")
    assert len(lines) == 3                                              # the header and two epochs
    for e, line in enumerate(lines[1:]):
        assert line.startswith(f"{e},")
        vals = [float(v) for v in line.replace("[", "").replace("]", "").split(",")[1:]]
        assert len(vals) == 11 and all(np.isfinite(vals)) and vals[0] > 0 and vals[5] > 0
    sd = torch.load(d / "1_fluidnet_uvp.pt", map_location="cpu", weights_only=True)
    assert sd and all(bool(torch.isfinite(v).all()) for v in sd.values())

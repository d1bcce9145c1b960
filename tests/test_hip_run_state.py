"""Exact restart on the GPU: a run that is stopped after an epoch, thrown away, rebuilt from scratch under another seed and
loaded from `fluidnet_state.pt` continues bit for bit as the run that never stopped.  Run A trains 4 epochs; run B trains 2
with save_state and is dropped; run B' is a new model, optimizer, scheduler, loaders and Trainer, loaded from B's file and
trained to epoch 4.  Every comparison is torch.equal / np.array_equal / ==: the step is deterministic, any difference is a bug.
MultiStepLR(milestones=[2, 3]) puts a milestone at the first resumed epoch."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

import run_state_worker as W

pytestmark = pytest.mark.gpu
DEV = W.DEV


# ---------------------------------------------------------------------------------------------------- 1, 2: U-Net, host loader
@pytest.mark.parametrize("precision,use_graph", [("fp32", False), ("mixed", True)], ids=["eager-fp32", "graph-mixed"])
def test_unet_resumes_bit_for_bit(tmp_path, precision, use_graph):
    kw = dict(precision=precision, use_graph=use_graph)
    a = W.straight("unet", str(tmp_path), **kw)
    d = W.stopped("unet", str(tmp_path), save_state=True, **kw)
    assert sorted(f for f in os.listdir(d) if "state" in f) == ["fluidnet_state.pt"]        # one file, no temporary left
    b = W.resumed("unet", d, **kw)
    assert W.same(a, b) == []
    assert int(a["step_count"]) == 8 and a["lr"] == 1e-3 * 0.25
    assert a["log"][2].endswith(",0.0005") and a["log"][3].endswith(",0.00025")


def test_without_the_state_file_a_restart_is_the_weights_only_one(tmp_path):
    """The default path, pinned: the weights of the last epoch, zero moments, step 0, and parse_restart_log's rate and
    milestones -- which is NOT the uninterrupted run (so the test above tests something)."""
    from pbml_mantle_convection_amd.multigpu import parse_restart_log
    a = W.straight("unet", str(tmp_path))
    d = W.stopped("unet", str(tmp_path))
    assert not os.path.exists(os.path.join(d, "fluidnet_state.pt"))
    epoch, lr, milestones = parse_restart_log(d + "/", list(W.MILESTONES))
    assert (epoch, lr, milestones) == (1, 1e-3, [1, 2])
    tr = W.build("unet", 77, d, epoch=epoch + 1, lr=lr, milestones=milestones, weights=os.path.join(d, "1_fluidnet_uvp.pt"))
    assert not bool(tr.exp_avg.any()) and not bool(tr.exp_avg_sq.any()) and int(tr.step_count.item()) == 0
    tr.train(W.EPOCHS)
    b = W.result(tr)
    assert b["log"][:2] == a["log"][:2]                                 # (B itself was run A's first half)
    assert "param" in W.same(a, b) and "exp_avg" in W.same(a, b) and "step_count" in W.same(a, b)
    assert b["log"][2].endswith(",0.001") and a["log"][2].endswith(",0.0005")               # the late milestone


# ---------------------------------------------------------------------------------------------------- 3: dropout + guard + graph
def test_dropout_guard_and_captured_step_resume_bit_for_bit(tmp_path):
    kw = dict(precision="mixed", use_graph=True)
    a = W.straight("drop", str(tmp_path), poison=(1, 1), **kw)
    d = W.stopped("drop", str(tmp_path), poison=(1, 1), save_state=True, **kw)
    st = torch.load(os.path.join(d, "fluidnet_state.pt"), map_location="cpu", weights_only=True)
    assert st["guard"]["skipped_seen"] == 1 and st["ranks"][0]["drop_step"] == 6 and int(st["optimizer"]["step_count"]) == 5
    b = W.resumed("drop", d, **kw)
    assert W.same(a, b) == []
    assert a["guard"]["skipped"] == 1 and a["guard"]["consecutive"] == 0 and a["drop_step"] == 12 and int(a["step_count"]) == 11


# ---------------------------------------------------------------------------------------------------- 4: the CLI, resident loop
def _equal(a, b, where=""):
    """Paths at which two nested states differ."""
    if isinstance(a, torch.Tensor):
        return [] if isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b) else [where]
    if isinstance(a, dict):
        if not isinstance(b, dict) or set(a) != set(b):
            return [where]
        return [w for k in a for w in _equal(a[k], b[k], f"{where}/{k}")]
    if isinstance(a, (list, tuple)):
        if not isinstance(b, (list, tuple)) or len(a) != len(b):
            return [where]
        return [w for i, (x, y) in enumerate(zip(a, b)) for w in _equal(x, y, f"{where}/{i}")]
    return [] if a == b else [where]


def test_cli_resident_run_restarts_bit_for_bit(golden, tmp_path, monkeypatch, capsys):
    import torch.distributed as dist
    from pbml_mantle_convection_amd import multigpu as G
    os.makedirs(tmp_path / "data")
    W.write_tree(golden("g18_newad_dataset"), str(tmp_path / "data"))
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)

    def cli(nn, *more):
        try:
            G.cli(["-net", "newfluidnet", "-l", "2", "-f", "8", "-r", "1", "-k", "3", "-p", "zeros", "-lt", "mass", "-pp", "1", "-s",
                   "1", "-ab", "10", "-b", "4", "-deb", "0", "-n", "0.1", "--data_dir", str(tmp_path / "data"), "--nn_root",
                   str(tmp_path / nn), "--precision", "fp32", "--resident", "1", "--use_graph", "1", "--save_state", "1", *more])
        finally:
            if dist.is_initialized():
                dist.destroy_process_group()
        runs = os.listdir(tmp_path / nn)
        assert len(runs) == 1
        return tmp_path / nn / runs[0]

    W.seed_all(10)
    da = cli("nnA", "--epochs", "4")
    W.seed_all(10)
    db = cli("nnB", "--epochs", "2")
    assert torch.load(db / "fluidnet_state.pt", weights_only=True)["header"]["epoch"] == 1
    W.seed_all(21)                                   # the restarted process has another seed: model, loader seeds, host streams
    capsys.readouterr()
    assert cli("nnB", "-rst", "1", "--epochs", "4") == db
    assert "[mantle]" not in capsys.readouterr().out
    sa, sb = (torch.load(d / "fluidnet_state.pt", map_location="cpu", weights_only=True) for d in (da, db))
    assert sa["header"]["epoch"] == 3 and sa["ranks"][0]["loaders"]["train_data"]["draw"] == 4 * 5
    assert _equal(sa, sb) == []
    wa, wb = (torch.load(d / "3_fluidnet_uvp.pt", map_location="cpu", weights_only=True) for d in (da, db))
    assert _equal(wa, wb) == [] and len(wa) > 0
    la, lb = (open(d / "fluidnet_uvpT.txt").read().strip().split("\n") for d in (da, db))
    assert len(la) == len(lb) == 5 and la[3:] == lb[3:] and la[3].startswith("2,") and la[4].startswith("3,")
    # a state file whose epoch is not the log's last: one line, then the weights-only restart
    st = dict(sb, header=dict(sb["header"], epoch=2))
    G.write_state_file(st, str(db / "fluidnet_state.pt"))
    cli("nnB", "-rst", "1", "--epochs", "5")
    out = capsys.readouterr().out
    assert out.count("[mantle]") == 1 and "epoch 2" in out and "epoch 3" in out
    assert len(open(db / "fluidnet_uvpT.txt").read().strip().split("\n")) == 6


# ---------------------------------------------------------------------------------------------------- 5: two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_resume_bit_for_bit(tmp_path):
    world = 2
    ctx = mp.get_context("forkserver")
    port = _free_port()
    procs = [ctx.Process(target=W.run, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.terminate()
            p.join(30)                                  # reaped before the next test opens the GPU
    assert not hung, f"ranks {hung} did not finish within 300 s"
    for p in procs:
        assert p.exitcode == 0, p.exitcode
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(world))
    for r in (r0, r1):
        assert r["differ"].tolist() == []                               # this rank's A equals its B'
        assert int(r["skipped"]) == 1 and int(r["step_count"]) == 11 and int(r["drop_step"]) == 12
        assert int(r["state_world"]) == 2 and int(r["state_epoch"]) == 1 and int(r["log_lines"]) == 4
    # one run directory, written by rank 0 alone: one state file, one weights file per epoch, one log line per epoch
    assert sorted(os.listdir(tmp_path / "run" / "B")) == ["0_fluidnet_uvp.pt", "1_fluidnet_uvp.pt", "2_fluidnet_uvp.pt",
                                                          "3_fluidnet_uvp.pt", "fluidnet_state.pt", "fluidnet_uvpT.txt"]
    assert np.array_equal(r0["param"], r1["param"]) and np.isfinite(r0["param"]).all()
    assert np.array_equal(r0["seeds"], r1["seeds"])                     # both ranks read the one file; it holds both entries
    assert r0["seeds"][0] != r0["seeds"][1]


# ---------------------------------------------------------------------------------------------------- 6: load under a graph
def test_loading_into_a_captured_trainer_is_in_place(tmp_path):
    tr = W.build("drop", 3, str(tmp_path), precision="mixed", use_graph=True)
    good, _ = W.drop_items()
    batches = [tr._prep(*tr._unpack(it)) for it in good]

    def steps(n, start):
        for i in range(start, start + n):
            tr.train_step(*batches[i % 3])
        torch.cuda.synchronize()

    steps(2, 0)
    ptrs = [t.data_ptr() for t in (tr.flat.param, tr.exp_avg, tr.exp_avg_sq, tr.step_count, tr._guard)]
    st = tr.state_dict()
    assert all(not t.is_cuda for t in (st["optimizer"]["param"], st["optimizer"]["exp_avg"], st["guard"]["record"]))
    assert st["ranks"][0]["drop_step"] == 2 and int(st["optimizer"]["step_count"]) == 2
    steps(2, 2)
    p4 = [t.clone() for t in (tr.flat.param, tr.exp_avg, tr.exp_avg_sq, tr.step_count)]
    assert not torch.equal(p4[0].cpu(), st["optimizer"]["param"])
    graph = tr._graph
    tr.load_state_dict(st)
    assert torch.equal(tr.flat.param.cpu(), st["optimizer"]["param"]) and tr.model_uvp.engine().dropout_step() == 2
    assert tr.flat.bound() and tr._graph is graph
    steps(2, 2)
    for got, want in zip((tr.flat.param, tr.exp_avg, tr.exp_avg_sq, tr.step_count), p4):
        assert torch.equal(got, want)
    assert ptrs == [t.data_ptr() for t in (tr.flat.param, tr.exp_avg, tr.exp_avg_sq, tr.step_count, tr._guard)]
    assert tr.model_uvp.engine().dropout_step() == 4


# ---------------------------------------------------------------------------------------------------- 7: refusals
def _small(width, precision, tmp_path):
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import Unet
    torch.manual_seed(4)
    m = Unet(2, 10, width, 3, torch.device(DEV), "gelu", "reflect", "mass", use_symm=True, repeats=1, f=3, p_pred=False)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[100], gamma=0.5)
    return Trainer(m, None, None, None, None, None, opt, sch, 0, 1, str(tmp_path) + "/", p_pred=False, network="unet",
                   loss_type="mass", precision=precision)


def test_states_that_cannot_continue_exactly_are_refused(tmp_path):
    a = _small(8, "fp32", tmp_path)
    st = a.state_dict()
    before = a.flat.param.clone()
    first = a.flat.names[0]
    with pytest.raises(ValueError, match=first.replace(".", r"\.")) as e:
        _small(16, "fp32", tmp_path).load_state_dict(st)                # another width
    assert str(tuple(a.flat.shapes[0])) in str(e.value)
    with pytest.raises(ValueError, match="precision.*fp32.*mixed"):
        _small(8, "mixed", tmp_path).load_state_dict(st)
    with pytest.raises(ValueError, match="world=2.*world=1"):
        a.load_state_dict(dict(st, header=dict(st["header"], world=2)))
    with pytest.raises(ValueError, match="version 99.*version 1"):
        a.load_state_dict(dict(st, header=dict(st["header"], version=99)))
    assert torch.equal(a.flat.param, before)                            # a refusal writes nothing
    b = _small(8, "fp32", tmp_path)
    with torch.no_grad():
        b.flat.param.add_(1.0)
    b.load_state_dict(st)                                               # the state itself is a good one
    assert torch.equal(b.flat.param, before) and b.flat.bound()

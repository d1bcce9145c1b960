"""Host side of the exact restart: the --save_state flag, the pure restart decision, the atomic state-file write, the host
RNG round trip and ResidentLoader.state() / load_state() on a device-free stand-in for the resident datasets."""
import os
import random

import numpy as np
import pytest
import torch


def test_save_state_flag_and_default():
    from pbml_mantle_convection_amd.multigpu import build_arg_parser
    p = build_arg_parser()
    assert p.parse_args([]).save_state == 0
    assert p.parse_args(["--save_state", "1"]).save_state == 1
    import inspect
    from pbml_mantle_convection_amd import multigpu as G
    assert inspect.signature(G.main).parameters["save_state"].default is False
    assert inspect.signature(G.Trainer.__init__).parameters["save_state"].default is False
    assert "save_state" not in inspect.signature(G.load_train_objs).parameters


def test_restart_decision():
    from pbml_mantle_convection_amd.multigpu import STATE_FILE, restart_decision
    assert restart_decision(None, 7) == (False, None)                   # no file: today's restart, silent
    assert restart_decision(7, 7) == (True, None)
    exact, msg = restart_decision(8, 7)                                 # killed between the state file and the log line
    assert exact is False and msg.startswith("[mantle]") and "8" in msg and "7" in msg and STATE_FILE in msg
    assert "\n" not in msg
    exact, msg = restart_decision(3, 7)
    assert exact is False and "3" in msg and "7" in msg


def test_state_file_write_is_atomic(tmp_path, monkeypatch):
    from pbml_mantle_convection_amd import multigpu as G
    path = str(tmp_path / G.STATE_FILE)
    G.write_state_file(dict(header=dict(epoch=1), t=torch.arange(5)), path)
    old = open(path, "rb").read()
    assert os.listdir(tmp_path) == [G.STATE_FILE]
    real = torch.save

    def failing(obj, f, *a, **k):
        real(obj, f, *a, **k)                                           # the temporary file exists, whole, when the write fails
        assert os.path.exists(f) and f != path and os.path.dirname(f) == str(tmp_path)
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", failing)
    with pytest.raises(OSError, match="disk full"):
        G.write_state_file(dict(header=dict(epoch=2), t=torch.arange(6)), path)
    assert open(path, "rb").read() == old
    assert os.listdir(tmp_path) == [G.STATE_FILE]
    monkeypatch.setattr(torch, "save", real)
    G.write_state_file(dict(header=dict(epoch=2), t=torch.arange(6)), path)
    st = G.read_state_file(path)                                        # (weights_only=True)
    assert st["header"]["epoch"] == 2 and torch.equal(st["t"], torch.arange(6))
    assert os.listdir(tmp_path) == [G.STATE_FILE]


def test_host_rng_round_trip_through_the_file(tmp_path):
    from pbml_mantle_convection_amd import multigpu as G
    torch.manual_seed(5)
    random.seed(6)
    np.random.seed(7)
    np.random.standard_normal(3)                                        # an odd count: the cached second gaussian is state too
    random.gauss(0, 1)
    path = str(tmp_path / "rng.pt")
    G.write_state_file(dict(rng=G.host_rng_state()), path)

    def draws():
        return torch.randperm(9).tolist(), torch.rand(2).tolist(), random.random(), random.gauss(0, 1), \
            np.random.standard_normal(2).tolist(), np.random.randint(0, 1 << 30, 3).tolist()

    want = draws()
    torch.manual_seed(1)
    random.seed(1)
    np.random.seed(1)
    G.set_host_rng_state(G.read_state_file(path)["rng"])
    assert draws() == want


class _Store:
    """What ResidentLoader needs of a resident dataset, without a device."""
    H, W, cy, device, noise = 6, 8, 3, torch.device("cpu"), True

    def __init__(self, n):
        self.n, self.noise_seed, self.is_init = n, 0, False

    def __len__(self):
        return self.n

    def store(self):
        return None


def test_resident_loader_state_round_trip():
    from pbml_mantle_convection_amd.datasetio import ResidentLoader, loader_seed
    a = ResidentLoader(_Store(10), _Store(4), batch_size=4, small_batch=2, seed=11, rank=1, world=2)
    a.set_cursor(2, 0xFFFFFFF0)                                         # a draw counter past 2^31 survives
    st = a.state()
    assert st == dict(seed=11, seed64=loader_seed(11, 1), step=2, draw=0xFFFFFFF0, noise_seed=[loader_seed(11, 1)] * 2)
    main, init = _Store(10), _Store(4)
    b = ResidentLoader(main, init, batch_size=4, small_batch=2, seed=98, rank=1, world=2)
    assert b.seed64 != a.seed64 and not torch.equal(b.build_table(3), a.build_table(3))
    cursor = b.cursor.data_ptr()
    b.load_state(st)
    assert b.state() == st and b.cursor.data_ptr() == cursor
    assert main.noise_seed == a.seed64 and init.noise_seed == a.seed64  # pushed to the datasets, as the constructor does
    assert torch.equal(b.build_table(3), a.build_table(3))
    assert b.cursor_state() == (2, 0xFFFFFFF0)


def _trainer(width=8, precision="fp32", drop=False, seed=4):
    """A Trainer on the host: the state's plumbing needs no kernel (no step is taken)."""
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import NewFluidNet, Unet
    torch.manual_seed(seed)
    dev = torch.device("cpu")
    if drop:
        m = NewFluidNet(3, 7, 8, 3, dev, "gelu", "zeros", "mae", use_symm=True, repeats=2, f=5, p_pred=True, drop_rate=0.25)
        kw = dict(network="newfluidnet", loss_type="mae", p_pred=True)
    else:
        m = Unet(2, 10, width, 3, dev, "gelu", "reflect", "mass", use_symm=True, repeats=1, f=3, p_pred=False)
        kw = dict(network="unet", loss_type="mass", p_pred=False)
    opt = torch.optim.Adam([{"params": m.parameters(), "lr": 1e-3, "weight_decay": 1e-4}])
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 3], gamma=0.5)
    return Trainer(m, None, None, None, None, None, opt, sch, "cpu", 1, "/tmp/", precision=precision, **kw)


@pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step")
def test_state_round_trip_through_the_file_is_in_place(tmp_path):
    from pbml_mantle_convection_amd import multigpu as G
    a = _trainer()
    a.exp_avg.normal_()
    a.exp_avg_sq.uniform_()
    a.step_count.fill_(7)
    a.scheduler.step()
    a.epoch_done = 1                                                    # as train() leaves it before the second scheduler step
    path = str(tmp_path / G.STATE_FILE)
    G.write_state_file(a.state_dict(), path)
    b = _trainer(seed=9)
    assert not torch.equal(b.flat.param, a.flat.param)
    ptrs = [t.data_ptr() for t in (b.flat.param, b.exp_avg, b.exp_avg_sq, b.step_count)]
    b.load_state(path)
    a.scheduler.step()                                                  # what A's train() does next
    assert torch.equal(b.flat.param, a.flat.param) and torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq)
    assert int(b.step_count) == 7 and b.start_epoch == 2 and b.get_lr() == a.get_lr() == 5e-4
    assert b.scheduler.state_dict() == a.scheduler.state_dict()
    assert b.flat.bound() and ptrs == [t.data_ptr() for t in (b.flat.param, b.exp_avg, b.exp_avg_sq, b.step_count)]
    assert torch.equal(next(b.model_uvp.parameters()).detach(), next(a.model_uvp.parameters()).detach())   # the views follow


def test_refusals_name_both_values():
    a = _trainer()
    st = a.state_dict()
    before = a.flat.param.clone()
    with pytest.raises(ValueError, match=r"conv\.0\.layers\.0\.weight.*\(7, 10, 3, 3\).*\(14, 10, 3, 3\)"):
        _trainer(width=16).load_state_dict(st)
    with pytest.raises(ValueError, match="precision='fp32'.*precision='mixed'"):
        _trainer(precision="mixed").load_state_dict(st)
    with pytest.raises(ValueError, match="network='unet'.*network='newfluidnet'"):
        _trainer(drop=True).load_state_dict(st)
    with pytest.raises(ValueError, match="world=2.*world=1"):
        a.load_state_dict(dict(st, header=dict(st["header"], world=2)))
    with pytest.raises(ValueError, match="version 99.*version 1"):
        a.load_state_dict(dict(st, header=dict(st["header"], version=99)))
    assert torch.equal(a.flat.param, before)


def test_restored_dropout_step_waits_for_the_engine_to_be_planned():
    """Engine.drop_state does not exist before configure(): a restored seed and step are kept until it does, and reach
    engines created later."""
    from pbml_mantle_convection_amd.engine import Engine
    seed = (1 << 63) + 12345
    a = _trainer(drop=True)
    st = a.state_dict()
    assert st["ranks"][0]["drop_step"] == 0 and st["ranks"][0]["drop_seed"] == a.drop_seed
    st["ranks"][0].update(drop_seed=seed, drop_step=5)
    b = _trainer(drop=True, seed=1)
    eng = b.model_uvp.engine()
    assert eng.drop_state is None and eng.dropout_step() == 0
    b.load_state_dict(st)
    assert (eng.dropout_step(), eng.dropout_seed(), b.model_uvp.dropout_seed(), b.drop_seed) == (5, seed, seed, seed)
    later = Engine(b.model_uvp._graph, "bf16")
    b.model_uvp.seed_engine(later)
    assert (later.dropout_step(), later.dropout_seed()) == (5, seed)
    b.model_uvp.set_dropout_seed(3)                                     # a new seed restarts the count, as before
    assert (eng.dropout_step(), eng.dropout_seed()) == (0, 3)


def test_a_scheduler_state_that_is_not_plain_data_is_refused_when_the_state_is_taken():
    a = _trainer()

    class Thing:
        pass

    a.scheduler.helper = Thing()                                        # (a scheduler's state_dict is its __dict__)
    with pytest.raises(TypeError, match="helper.*Thing"):
        a.state_dict()

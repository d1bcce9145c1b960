"""Host side of the resident epoch loop (`datasetio.epoch_table`, `epoch_steps`, the noise generator's host twin
`mc_newad_noise_host`, and the `--resident` / `-n` plumbing of the CLI).  No GPU."""
import os

import numpy as np
import pytest
import torch


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


N, B, SB, NI = 23, 6, 2, 5


def _table(**kw):
    from pbml_mantle_convection_amd.datasetio import epoch_table
    a = dict(seed=7, epoch=0, rank=0)
    a.update(kw)
    return epoch_table(N, B, SB, NI, **a)


def test_epoch_table_main_entries_are_a_shuffled_epoch():
    t = _table()
    steps = N // (B - SB)
    assert t.dtype == torch.int32 and tuple(t.shape) == (steps, B)
    main = t[t >= 0]
    assert main.numel() == steps * (B - SB) and len(set(main.tolist())) == main.numel()
    assert int(main.max()) < N
    assert main.tolist() != sorted(main.tolist())                       # shuffled


def test_epoch_table_init_entries_per_row():
    t = _table()
    cols = []
    for row in t:
        neg = row[row < 0]
        assert neg.numel() == SB and len(set(neg.tolist())) == SB       # small_batch init items, distinct within the row
        assert int((-neg - 1).max()) < NI and int((-neg - 1).min()) >= 0
        cols.append(tuple(torch.nonzero(row < 0).flatten().tolist()))
    assert len(set(cols)) > 1                                           # each row is permuted as a whole


def test_epoch_table_is_a_function_of_seed_epoch_rank():
    assert torch.equal(_table(), _table())
    assert not torch.equal(_table(), _table(epoch=1))
    assert not torch.equal(_table(), _table(rank=1))
    assert not torch.equal(_table(), _table(seed=8))


def test_steps_and_no_init_set():
    from pbml_mantle_convection_amd.datasetio import epoch_steps, epoch_table, validate_table
    for n in (23, 24, 25, 4, 3):
        for b, sb in ((6, 2), (4, 0), (5, 1)):
            t = epoch_table(n, b, sb, NI, seed=1)
            assert t.shape[0] == n // (b - sb) == epoch_steps([n], b, sb)
    t = epoch_table(N, B, 0, 0, seed=3)
    assert tuple(t.shape) == (N // B, B) and int(t.min()) >= 0
    assert sorted(t.flatten().tolist()) != t.flatten().tolist()
    validate_table(t, N, 0)
    with pytest.raises(IndexError):
        validate_table(t, int(t.max()), 0)                              # an entry past the main store
    with pytest.raises(IndexError):
        validate_table(torch.tensor([[0, -NI - 1]]), N, NI)             # ... and one past the init store
    with pytest.raises(IndexError):
        validate_table(torch.tensor([[[0, -1]]]), N, NI)                # a pair from two stores
    with pytest.raises(ValueError):
        epoch_table(N, B, NI + 1, NI)                                   # more init items per row than the init set has
    with pytest.raises(ValueError):
        epoch_table(N, B, B, NI)


def test_adtime_pairs_with_a_multiple_of_eight_become_init_pairs():
    from pbml_mantle_convection_amd.datasetio import epoch_table
    # three simulations of 12, 9 and 11 snapshots (the counter runs on across them, as in ADTimeDataset)
    pairs, init, c = [], [], 0
    for n in (12, 9, 11):
        for i in range(n):
            if i < n - 2:
                pairs.append([c, c + 1])
                if i == 0:
                    init.append([c, c + 1])
            c += 1
    kw = dict(seed=5, epoch=2, rank=0)
    idx = epoch_table(len(pairs), 4, **kw)
    t = epoch_table(len(pairs), 4, pairs=pairs, pairs_init=init, **kw)
    assert tuple(t.shape) == (len(pairs) // 4, 4, 2) and t.dtype == torch.int32
    src = torch.tensor(pairs)[idx.long()]
    replaced = src[..., 0] % 8 == 0
    assert bool(replaced.any()) and not bool(replaced.all())
    assert torch.equal(t[~replaced].long(), src[~replaced])             # no other pair is touched
    init_set = {tuple(p) for p in init}
    assert all(tuple(p) in init_set for p in t[replaced].tolist())
    for p in t.reshape(-1, 2).tolist():                                 # every pair with i0 % 8 == 0 is an init pair
        if p[0] % 8 == 0:
            assert tuple(p) in init_set
    drawn = set()                                                       # drawn, not one fixed pair: 4 replaced pairs per epoch,
    for e in range(8):                                                  # 3 init pairs; one value 32 times has probability 3^-31
        te = epoch_table(len(pairs), 4, pairs=pairs, pairs_init=init, seed=5, epoch=e)
        se = torch.tensor(pairs)[epoch_table(len(pairs), 4, seed=5, epoch=e).long()]
        drawn |= {tuple(p) for p in te[se[..., 0] % 8 == 0].tolist()}
    assert len(drawn) > 1 and drawn <= init_set


def test_ranks_with_shards_of_n_and_n_plus_one_run_the_same_steps():
    from pbml_mantle_convection_amd.datasetio import epoch_steps, epoch_table
    from pbml_mantle_convection_amd.multigpu import shard_range
    b, sb = 6, 1
    for n in (19, 20, 24):                                              # n = 19: 19 // 5 = 3 but 20 // 5 = 4
        sizes = [n, n + 1]
        steps = epoch_steps(sizes, b, sb)
        assert steps == n // (b - sb)
        tabs = [epoch_table(sizes[r], b, sb, NI, seed=1, epoch=0, rank=r, steps=steps) for r in (0, 1)]
        assert tabs[0].shape == tabs[1].shape == (steps, b)
    spans = [shard_range(41, 2, r) for r in (0, 1)]
    assert len({epoch_steps([hi - lo for lo, hi in spans], b, sb) for _ in (0, 1)}) == 1
    with pytest.raises(ValueError):
        epoch_table(19, b, sb, NI, steps=4)


def test_noise_twin_is_uniform_inside_the_open_interval():
    """10^5 draws: strictly inside (-1e-5, 1e-5); the mean of n uniform draws of variance a^2 / 3 has standard deviation
    a / sqrt(3 n), and the bound is five of them (derived, not measured)."""
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    seed, n = (0x1234, 0x4C4F4144), 100000
    d = np.array([lib.mc_newad_noise_host(seed[0], seed[1], 3, 5, p) for p in range(n)], dtype=np.float64)
    assert d.max() < 1e-5 and d.min() > -1e-5
    assert abs(d.mean()) <= 5 * 1e-5 / np.sqrt(3 * n)
    assert d.max() > 0.999e-5 and d.min() < -0.999e-5 and len(np.unique(d)) > 0.99 * n
    f = lib.mc_newad_noise_host
    same = f(seed[0], seed[1], 3, 5, 17)
    assert same == f(seed[0], seed[1], 3, 5, 17)
    assert len({same, f(seed[0], seed[1], 4, 5, 17), f(seed[0], seed[1], 3, 6, 17), f(seed[0], seed[1], 3, 5 | 0x80000000, 17),
                f(seed[0] + 1, seed[1], 3, 5, 17), f(seed[0], seed[1] + 1, 3, 5, 17), f(seed[0], seed[1], 3, 5, 18)}) == 7
    # the formula, restated: word 0 of Philox with counter (pixel, item, draw, tag)
    import ctypes as C
    ctr, key, out = (C.c_uint32 * 4)(17, 5, 3, 0x6E6F6973), (C.c_uint32 * 2)(*seed), (C.c_uint32 * 4)()
    lib.mc_philox4x32(ctr, key, out)
    u = ((out[0] >> 8) + 0.5) * 2.0 ** -24
    assert same == np.float32(np.float32(2 * u - 1) * np.float32(1e-5))


def test_cli_resident_flag_and_noise_reach_the_datasets(golden, tmp_path, monkeypatch):
    from pbml_mantle_convection_amd import multigpu as G
    p = G.build_arg_parser()
    assert p.parse_args([]).resident == 0 and p.parse_args(["--resident", "1"]).resident == 1
    with pytest.raises(ValueError, match="synthetic"):
        G.cli(["-net", "newfluidnet", "-b", "2", "--resident", "1", "--synthetic", "4", "16", "16", "--nn_root", str(tmp_path / "nn")])
    with pytest.raises(ValueError, match="synthetic"):
        G.main(0, 1, 1, 1, 2, str(tmp_path) + "/", "", 2, 7, 8, 3, "gelu", "zeros", "mass", True, 1, 3, [5], {}, {}, {}, {},
               synthetic=dict(n=4, H=16, W=16), resident=True)

    class Reached(Exception):
        pass

    seen = {}

    def fake(*a, **k):
        seen.update(k)
        raise Reached

    os.makedirs(tmp_path / "data")
    _write_tree(golden("g18_newad_dataset"), str(tmp_path / "data"))
    monkeypatch.setattr(G, "ddp_setup", lambda *a, **k: None)
    monkeypatch.setattr(G, "build_model", lambda *a, **k: torch.nn.Linear(2, 2))
    monkeypatch.setattr(G, "NewADDataset", fake)
    argv = ["-net", "newfluidnet", "-l", "2", "-f", "8", "-r", "1", "-k", "3", "-p", "zeros", "-lt", "mass", "-pp", "1", "-s", "1",
            "-ab", "10", "-b", "3", "-deb", "0", "--data_dir", str(tmp_path / "data"), "--nn_root", str(tmp_path / "nn")]
    for extra, want in ((["-n", "0.1"], 0.1), ([], 0.0), (["-n", "0.1", "--resident", "1"], 0.1)):
        seen.clear()
        with pytest.raises(Reached):
            G.cli(argv + extra)
        assert seen["noise"] == want

"""No GPU: argument checks of the series-scoring entry points, load_series on a tiny directory in the reference's layout, the
numpy reference on fields with known answers, the command line parser and the csv / npz writers."""
import csv
import os

import numpy as np
import pytest
import torch

import series_score_ref as R

H0, W0 = 6, 7


# ---- argument checks through the C ABI (nothing is launched, so the pointers are never followed) ----------------------------------
P = 4096            # any non-null address


def build_input(h=5, w=5, b=2, n_items=3, T=P, stride=None, cursor=P):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_series_build_input(T, h * w if stride is None else stride, P, P, P, P, P, P, P, cursor, n_items, 4, 2, b, h, w, P, None)


def score(h=5, w=5, b=2, n_items=3, rows=P, uvs=None, stride=None):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_series_score(P, P, h * w if uvs is None else uvs, P, P, h * w if stride is None else stride, P, P, P, P, P, n_items,
                                    4, 2, b, h, w, rows, None)


def finalize(h=5, w=5, b=2, n_items=3, table=P):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_series_score_finalize(P, P, P, n_items, 4, b, h, w, table, P, None)


@pytest.mark.parametrize("fn", [build_input, score, finalize])
def test_entry_points_refuse_bad_arguments(fn):
    from pbml_mantle_convection_amd import _lib as L
    EINVAL = -1
    for kw in (dict(h=2), dict(w=2), dict(b=0), dict(b=65536), dict(n_items=0)):
        assert fn(**kw) == EINVAL, kw
    null = {build_input: dict(T=None), score: dict(rows=None), finalize: dict(table=None)}[fn]
    assert fn(**null) == EINVAL
    with pytest.raises(L.MantleHipError):
        L.call("mc_series_set_cursor", None, 0, 3, None)


def test_strides_and_cursor_rows_are_checked():
    from pbml_mantle_convection_amd import _lib as L
    assert build_input(stride=24) == -1 and score(uvs=24) == -1 and score(stride=24) == -1
    assert build_input(cursor=None) == -1
    lib = L.load()
    assert lib.mc_series_set_cursor(P, -1, 3, None) == -1 and lib.mc_series_set_cursor(P, 4, 3, None) == -1
    assert lib.mc_series_set_cursor(P, 0, 0, None) == -1


# ---- load_series -----------------------------------------------------------------------------------------------------------------
def write_sim(root, an, num, n, seed, grid_shift=0.0):
    d = os.path.join(root, an, f"sim_{num}")
    os.makedirs(d)
    rng = np.random.RandomState(seed)
    xs = np.linspace(0.1, 3.9, W0) + grid_shift
    ys = np.linspace(0.05, 0.95, H0)
    torch.save(torch.from_numpy(np.broadcast_to(xs[None, :], (H0, W0)).copy()), os.path.join(d, "xc.pt"))
    torch.save(torch.from_numpy(np.broadcast_to(ys[:, None], (H0, W0)).copy()), os.path.join(d, "yc.pt"))
    data = {k: rng.standard_normal((n, 1, H0, W0)) for k in "uvT"}
    for k, a in data.items():
        torch.save(torch.from_numpy(a), os.path.join(d, f"e1_{k}prev_data.pt"))
    return data


@pytest.fixture()
def tree(tmp_path):
    root = str(tmp_path)
    sims = [(3, "cv", 1.5, 1e6, 10.0, 0.0, 0.0, 0), (7, "cv", 4.0, 1e8, 60.0, 0.0, 0.0, 0), (9, "train", 2.0, 1e7, 30.0, 0.0, 0.0, 0)]
    torch.save(sims, os.path.join(root, "sims.pt"))
    data = {3: write_sim(root, "cv", 3, 3, 1), 7: write_sim(root, "cv", 7, 4, 2), 9: write_sim(root, "train", 9, 2, 3, grid_shift=0.01)}
    return root, data


def test_load_series_layout(tree):
    from pbml_mantle_convection_amd.evaluate import load_series
    root, data = tree
    s = load_series(root, "cv")
    assert s["T"].shape == (7, H0, W0) and s["T"].dtype == np.float32 and s["sim_ids"] == [3, 7]
    assert s["sim"].tolist() == [0, 0, 0, 1, 1, 1, 1] and s["prev"].tolist() == [-1, 0, 1, -1, 3, 4, 5]
    assert s["raq"].tolist() == [1.5, 4.0] and s["fkt"].tolist() == [1e6, 1e8] and s["fkp"].tolist() == [10.0, 60.0]
    assert np.array_equal(s["u"][:3], data[3]["u"][:, 0].astype(np.float32)) and np.array_equal(s["v"][3:], data[7]["v"][:, 0].astype(np.float32))
    assert np.array_equal(s["T"][3:], data[7]["T"][:, 0].astype(np.float32))
    # the mesh training saw: wall coordinates in the first / last column of xc and row of yc
    assert (s["xc"][:, 0] == 0).all() and (s["xc"][:, -1] == 4).all() and (s["yc"][0] == 0).all() and (s["yc"][-1] == 1).all()
    assert s["xc"].shape == (H0, W0) and 0 < s["xc"][2, 1] < s["xc"][2, 2] < 4


def test_load_series_every_and_selection(tree):
    from pbml_mantle_convection_amd.evaluate import load_series
    root, data = tree
    s = load_series(root, "cv", every=2)
    assert s["sim"].tolist() == [0, 0, 1, 1] and s["prev"].tolist() == [-1, 0, -1, 2]         # the preceding KEPT snapshot
    assert np.array_equal(s["u"], np.concatenate([data[3]["u"][::2, 0], data[7]["u"][::2, 0]]).astype(np.float32))
    one = load_series(root, "cv", sims=[7])
    assert one["sim_ids"] == [7] and one["sim"].tolist() == [0] * 4 and one["prev"].tolist() == [-1, 0, 1, 2] and one["raq"].tolist() == [4.0]
    with pytest.raises(ValueError):
        load_series(root, "cv", sims=[5])
    with pytest.raises(ValueError):
        load_series(root, "cv", every=0)


def test_load_series_refuses_mixed_meshes(tree):
    from pbml_mantle_convection_amd.evaluate import load_series
    root, _ = tree
    sims = torch.load(os.path.join(root, "sims.pt"), weights_only=True)
    write_sim(root, "cv", 11, 2, 4, grid_shift=0.01)
    torch.save(list(sims) + [(11, "cv", 2.0, 1e7, 30.0, 0.0, 0.0, 0)], os.path.join(root, "sims.pt"))
    with pytest.raises(ValueError, match="one depth grid"):
        load_series(root, "cv")
    assert load_series(root, "cv", sims=[3, 7])["sim_ids"] == [3, 7]


def test_previous_snapshots_and_inverse_scale():
    from pbml_mantle_convection_amd import evaluate as E
    from pbml_mantle_convection_amd.scaler import velocity_scaler
    assert E.previous_snapshots([0, 1, 0, 0, 1]).tolist() == [-1, -1, 0, 2, 1]
    inv = E.inverse_velocity_scale([1.5, 4.0], [1e6, 1e8], [10.0, 60.0])
    assert inv.dtype == np.float32
    want = [np.float32(1.0 / velocity_scaler(np.float64(r), np.float64(t), np.float64(p))) for r, t, p in ((1.5, 1e6, 10.0), (4.0, 1e8, 60.0))]
    assert inv.tolist() == [float(w) for w in want]


# ---- the numpy reference on fields with known answers ----------------------------------------------------------------------------
def stream_uv(psi):
    """u = d psi / dy, v = -d psi / dx by central differences of psi [H+2, W+2]: div(u, v) of the contract vanishes identically."""
    return 0.5 * (psi[2:, 1:-1] - psi[:-2, 1:-1]), -0.5 * (psi[1:-1, 2:] - psi[1:-1, :-2])


def test_reference_known_answers():
    rng = np.random.RandomState(5)
    N, H, W = 3, 9, 12
    u = rng.standard_normal((N, H, W)).astype(np.float32)
    v = rng.standard_normal((N, H, W)).astype(np.float32)
    sim, prev = np.array([0, 0, 1]), np.array([-1, 0, -1])
    inv = np.array([0.37, 2.5], dtype=np.float32)
    idx = [0, 1, 2]
    # a perfect prediction: u_hat = ut exactly
    uh = np.stack([u[s] * inv[sim[s]] for s in idx])
    vh = np.stack([v[s] * inv[sim[s]] for s in idx])
    assert uh.dtype == np.float32
    table, profile, gate, _ = R.score(uh, vh, u, v, sim, prev, inv, idx)
    assert (table[:, [0, 1, 6, 7]] == 0).all() and (profile == 0).all() and (gate[:, [0, 1]] == 0).all()
    for j, s in enumerate(idx):
        assert table[j, 4] == float(np.abs(u[s] * inv[sim[s]]).max()) and table[j, 5] == float(np.abs(v[s] * inv[sim[s]]).max())
    assert np.array_equal(table[:, 8], table[:, 9]) and (table[:, 9] > 0).all()           # prediction == truth: the same residual
    # baselines: NaN for a first snapshot, the mean |difference of the scaled fields| elsewhere
    assert np.isnan(table[[0, 2]][:, 2:4]).all()
    d = np.abs((u[1] * inv[0]).astype(np.float64) - (u[0] * inv[0]).astype(np.float64))
    assert abs(table[1, 2] - d.sum() / (H * W)) <= 1e-15 * d.sum() and table[1, 3] > 0
    # a constant offset: every error column is the offset
    t2, p2, _, _ = R.score(uh + np.float32(0.5), vh, u, v, sim, prev, inv, idx)
    assert np.allclose(t2[:, 0], 0.5, rtol=0, atol=1e-6) and np.allclose(t2[:, 6], 0.5, rtol=0, atol=1e-6) and (t2[:, 1] == 0).all()
    assert np.allclose(p2[:, 0], 0.5, rtol=0, atol=1e-6) and p2.shape == (3, 2, H)
    assert np.allclose(t2[:, 8], table[:, 8], rtol=0, atol=1e-6)      # an offset carries no divergence (but its f32 rounding)


def test_reference_mass_of_a_stream_function_velocity():
    rng = np.random.RandomState(6)
    H, W = 8, 11
    sim, prev, inv = np.array([0]), np.array([-1]), np.array([1.0], dtype=np.float32)
    # integer stream function: u, v are multiples of 0.5, exact in f32, and the residual is exactly zero
    psi = rng.randint(-50, 50, (H + 2, W + 2)).astype(np.float64)
    u, v = (a.astype(np.float32)[None] for a in stream_uv(psi))
    table, _, _, _ = R.score(np.zeros_like(u), np.zeros_like(v), u, v, sim, prev, inv, [0])
    assert table[0, 9] == 0.0 and table[0, 8] == 0.0 and table[0, 4] == float(np.abs(u).max())
    # smooth stream function: only the f32 rounding of u, v is left, four roundings of at most 2^-25 max|.| each, halved
    y, x = np.meshgrid(np.linspace(0, 1, H + 2), np.linspace(0, 4, W + 2), indexing="ij")
    u64, v64 = stream_uv(np.sin(3 * y) * np.cos(2 * x + 0.3) * 40.0)
    u, v = u64.astype(np.float32)[None], v64.astype(np.float32)[None]
    table, _, _, _ = R.score(np.zeros_like(u), np.zeros_like(v), u, v, sim, prev, inv, [0])
    bound = 2.0 * 2.0 ** -25 * max(np.abs(u).max(), np.abs(v).max()) + 1e-13
    print(f"mass_true {table[0, 9]:.3e} bound {bound:.3e} against max|u| {np.abs(u).max():.3e}")
    assert 0 < table[0, 9] <= bound
    # a velocity that is NOT solenoidal is seen
    table, _, _, _ = R.score(np.zeros_like(u), np.zeros_like(v), u, u, sim, prev, inv, [0])
    assert table[0, 9] > 1e3 * bound


def test_reference_permuted_and_repeated_list():
    rng = np.random.RandomState(7)
    N, H, W = 4, 5, 6
    u, v = (rng.standard_normal((N, H, W)).astype(np.float32) for _ in range(2))
    uh, vh = (rng.standard_normal((N, H, W)).astype(np.float32) for _ in range(2))
    sim, prev, inv = np.array([0, 0, 1, 1]), np.array([-1, 0, -1, 2]), np.array([0.5, 3.0], dtype=np.float32)
    full, prof, _, _ = R.score(uh, vh, u, v, sim, prev, inv, [0, 1, 2, 3])
    idx = [3, 1, 1, 0]
    t, p, _, _ = R.score(uh[idx], vh[idx], u, v, sim, prev, inv, idx)
    assert np.array_equal(t, full[idx], equal_nan=True) and np.array_equal(p, prof[idx])


# ---- the command line and the writers --------------------------------------------------------------------------------------------
def test_cli_parser():
    from pbml_mantle_convection_amd.evaluate import build_arg_parser
    a = build_arg_parser().parse_args("--out o --data_dir d".split())
    assert (a.levels, a.c_h, a.repeats, a.kernel, a.r_p, a.act_fn, a.loss_type) == (5, 16, 6, 5, "zeros", "gelu", "mass")
    assert (a.an, a.sims, a.every, a.batch, a.precision, a.graph, a.synthetic, a.weights) == ("cv", None, 1, 32, None, 1, None, None)
    a = build_arg_parser().parse_args("--weights w.pt -l 3 -f 8 -r 2 -k 3 -p reflect -a relu -lt mae --data_dir d --an train --sims 3 7 "
                                      "--every 4 --batch 8 --precision bf16 --graph 0 --out o --synthetic 5 64 90".split())
    assert (a.weights, a.levels, a.c_h, a.repeats, a.kernel, a.r_p, a.act_fn, a.loss_type) == ("w.pt", 3, 8, 2, 3, "reflect", "relu", "mae")
    assert (a.an, a.sims, a.every, a.batch, a.precision, a.graph, a.synthetic) == ("train", [3, 7], 4, 8, "bf16", 0, [5, 64, 90])
    with pytest.raises(SystemExit):
        build_arg_parser().parse_args(["--data_dir", "d"])              # --out is required


def test_writers_and_summary(tmp_path):
    from pbml_mantle_convection_amd import evaluate as E
    assert E.SCORE_NAMES == R.NAMES
    rng = np.random.RandomState(8)
    table = rng.uniform(0.1, 1.0, (5, 10))
    table[0, 2:4] = table[3, 2:4] = np.nan
    profile = rng.uniform(0, 1, (5, 2, 4))
    idx, sim = np.array([4, 0, 1, 2, 3]), np.array([1, 0, 0, 1, 1])
    npz, path = E.write_scores(str(tmp_path / "o"), table, profile, idx, sim, sim_ids=[3, 7])
    z = np.load(npz)
    assert set(z.files) == {"table", "names", "profile", "idx", "sim"} and z["names"].tolist() == list(R.NAMES)
    assert np.array_equal(z["table"], table, equal_nan=True) and np.array_equal(z["profile"], profile)
    assert z["idx"].tolist() == idx.tolist() and z["sim"].tolist() == [7, 3, 3, 7, 7]
    with open(path) as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["item", "snapshot", "sim"] + list(R.NAMES) and len(rows) == 6
    assert rows[1][:3] == ["0", "4", "7"] and rows[1][5] == "nan" and float(rows[2][3]) == table[1, 0]          # repr: exact round trip
    assert all(float(rows[1 + j][3 + q]) == table[j, q] for j in range(5) for q in range(10) if not np.isnan(table[j, q]))
    s = E.summarise(table, sim, sim_ids=[3, 7])
    assert [d["sim"] for d in s] == [3, 7] and [d["snapshots"] for d in s] == [2, 3]
    assert s[0]["mae_u"] == table[[1, 2], 0].mean() and s[1]["base_u"] == table[4, 2]                          # NaN baselines left out
    assert s[0]["base_over_mae_u"] == s[0]["base_u"] / s[0]["mae_u"] and s[1]["base_over_mae_v"] == s[1]["base_v"] / s[1]["mae_v"]
    with pytest.raises(ValueError):
        E.write_scores(str(tmp_path / "o"), table[:4], profile, idx, sim)


def test_scorer_refuses_other_networks():
    from pbml_mantle_convection_amd.evaluate import SeriesScorer
    from pbml_mantle_convection_amd.pytorch_networks_convae import FluidNet, Unet
    unet = Unet(2, 11, 8, 4, torch.device("cpu"), "gelu", "reflect", "mae", use_symm=True, repeats=1, f=3, p_pred=True)
    with pytest.raises(NotImplementedError):
        SeriesScorer(unet, "cpu")
    fluid = FluidNet(2, 7, 8, 3, None, "gelu", "zeros", "curl", use_symm=True, repeats=1, f=3, p_pred=False)
    with pytest.raises(NotImplementedError):
        SeriesScorer(fluid, "cpu")


def test_ts_without_advection_net_needs_one_step():
    from pbml_mantle_convection_amd.pytorch_networks_convae import TS
    with pytest.raises(ValueError, match="KeyError"):
        TS(torch.nn.Identity(), None, "cpu", ts=2, net="newfluidnet")
    ts = TS(torch.nn.Identity(), None, "cpu", ts=1, net="newfluidnet")
    assert ts.ad is None and ts.ts == 1

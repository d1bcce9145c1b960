"""CPU-only checks of the ensemble rollout: the mc_rollout_* entry points are declared, exported, bound and validate their
arguments without a device; parameter files, normalisation, t_end broadcasting, the history's column names and the
state()/load_state() round trip on host tensors."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_EINVAL = -1
A = 0x10000          # an aligned address that is never dereferenced: validation fails before any launch
ENTRY_POINTS = ("mc_rollout_blocks", "mc_rollout_dx_min", "mc_rollout_dt", "mc_rollout_step", "mc_rollout_finalize",
                "mc_rollout_set_cursor")


def test_entry_points_declared_exported_and_bound():
    from pbml_mantle_convection_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "mantle_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mc_rollout_[a-z0-9_]+)\s*\(", src))
    assert declared == set(ENTRY_POINTS)
    lib = L.load()
    for name in ENTRY_POINTS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    from pbml_mantle_convection_amd import build_ext
    assert "rollout.hip" in build_ext.SOURCES


def _dx(xc=A, h=8, w=9, out=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_rollout_dx_min(xc, h, w, out, None)


def _dt(u=A, v=A, uvs=72, vs=A, dxm=A, t=A, te=A, b=2, h=8, w=9, ws=A, dt=A, flags=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_rollout_dt(u, v, uvs, vs, dxm, t, te, b, h, w, 0.1, ws, dt, flags, None)


def _step(u=A, v=A, uvs=72, vs=A, T=A, raq=A, xc=A, yc=A, dt=A, flags=A, b=2, h=8, w=9, Tn=2 * A, part=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_rollout_step(u, v, uvs, vs, T, raq, xc, yc, dt, flags, b, h, w, Tn, part, None)


def _fin(part=A, dt=A, flags=A, te=A, t=A, steps=A, cursor=A, hist=A, n_steps=4, b=2, h=8, w=9):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_rollout_finalize(part, dt, flags, te, t, steps, cursor, hist, n_steps, b, h, w, None)


def _cur(cursor=A, row=0, n_steps=4):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_rollout_set_cursor(cursor, row, n_steps, None)


def test_rollout_entry_points_validate_arguments_without_gpu():
    from pbml_mantle_convection_amd import _lib as L
    sizes = (dict(b=0), dict(b=-1), dict(b=65536), dict(h=4), dict(w=4), dict(h=0), dict(w=-3))
    for kw in (dict(xc=None), dict(out=None), dict(h=4), dict(w=4)):
        assert _dx(**kw) == MC_EINVAL, kw
    for kw in (dict(u=None), dict(v=None), dict(dxm=None), dict(t=None), dict(te=None), dict(ws=None), dict(dt=None),
               dict(flags=None), dict(uvs=71)) + sizes:
        assert _dt(**kw) == MC_EINVAL, kw
    for kw in (dict(u=None), dict(v=None), dict(T=None), dict(raq=None), dict(xc=None), dict(yc=None), dict(dt=None),
               dict(flags=None), dict(Tn=None), dict(part=None), dict(uvs=71), dict(Tn=A)) + sizes:       # (Tn=A: in place)
        assert _step(**kw) == MC_EINVAL, kw
    for kw in (dict(part=None), dict(dt=None), dict(flags=None), dict(te=None), dict(t=None), dict(steps=None),
               dict(cursor=None), dict(hist=None), dict(n_steps=0), dict(n_steps=-2)) + sizes:
        assert _fin(**kw) == MC_EINVAL, kw
    for kw in (dict(cursor=None), dict(n_steps=0), dict(row=-1), dict(row=5)):                        # a cursor beyond n_steps
        assert _cur(**kw) == MC_EINVAL, kw
    assert L.call("mc_rollout_blocks", 4, 9) == MC_EINVAL and L.call("mc_rollout_blocks", 9, 4) == MC_EINVAL
    with pytest.raises(L.MantleHipError):
        L.call("mc_rollout_set_cursor", None, 0, 4, None)


def test_rollout_blocks_depend_on_the_grid_alone():
    from pbml_mantle_convection_amd import _lib as L
    nb = lambda h, w: L.call("mc_rollout_blocks", h, w)  # noqa: E731
    assert nb(5, 6) == 1 and nb(9, 70) == 3 and nb(33, 130) == 17
    assert nb(128, 506) == 128 == nb(4096, 4096)            # capped: the blocks grid-stride


def test_params_csv_and_normalisation(tmp_path):
    from pbml_mantle_convection_amd import rollout as R
    from pbml_mantle_convection_amd.datasetio import normalise_parameters
    p = tmp_path / "params.csv"
    p.write_text("raq,fkt,fkp\n# a comment\n1.5, 1e6, 10\n\n2.5,1e7,30   # trailing\n4.0,1e8,60\n")
    paras = R.parse_params_csv(str(p))
    assert paras.dtype == np.float64 and paras.tolist() == [[1.5, 1e6, 10.0], [2.5, 1e7, 30.0], [4.0, 1e8, 60.0]]
    nd = R.normalise_params(paras)
    assert nd.shape == (3, 3)
    # the constants of the reference's non_dimensionalize_raq / _fkt / _fkv
    want = np.stack([(paras[:, 0] - 0.12624371) / (9.70723344 - 0.12624371),
                     (np.log10(paras[:, 1]) - 6.00352841978384) / (9.888820429862925 - 6.00352841978384),
                     (np.log10(paras[:, 2]) - 0.005251646002323797) / (1.9927988938926755 - 0.005251646002323797)], 1)
    np.testing.assert_allclose(nd, want, rtol=1e-15, atol=0)
    assert np.allclose(nd[1], normalise_parameters(2.5, 1e7, 30.0))
    for bad in ("1.0,2.0\n", "1.0,1e6,abc\n", "1.0,-1e6,10\n", "# nothing\n"):
        p.write_text(bad)
        with pytest.raises(ValueError):
            R.parse_params_csv(str(p))


def test_t_end_is_broadcast():
    from pbml_mantle_convection_amd import rollout as R
    t = R.broadcast_t_end(None, 3)
    assert t.dtype == torch.float64 and t.tolist() == [float("inf")] * 3
    assert R.broadcast_t_end(2e-4, 3).tolist() == [2e-4] * 3
    assert R.broadcast_t_end(torch.tensor([1e-4], dtype=torch.float64), 2).tolist() == [1e-4] * 2
    assert R.broadcast_t_end([1e-4, float("inf"), 3e-4], 3).tolist() == [1e-4, float("inf"), 3e-4]
    assert R.broadcast_t_end(np.float32(0.5), 2).dtype == torch.float64
    for bad in ([1.0, 2.0], float("nan")):
        with pytest.raises(ValueError):
            R.broadcast_t_end(bad, 3)


def test_history_column_names():
    from pbml_mantle_convection_amd import rollout as R
    assert R.HIST_NAMES == ("t", "dt", "T_mean", "v_rms", "Nu_bot", "Nu_top", "T_min", "T_max")


def test_state_roundtrip_on_cpu_tensors():
    from pbml_mantle_convection_amd import rollout as R
    T0, xc, yc = R.synthetic_ensemble(3, 6, 7, seed=4)
    assert T0.shape == (3, 1, 6, 7) and (T0[:, 0, 0] == 1).all() and (T0[:, 0, -1] == 0).all()
    assert xc[0, 0] == 0 and xc[0, -1] == 4 and yc[0, 0] == 0 and yc[-1, 0] == 1
    st = dict(T=torch.from_numpy(T0), t=torch.tensor([0.0, 1e-3, 0.1 + 0.2], dtype=torch.float64),
              t_end=torch.tensor([float("inf"), 2e-3, 0.25], dtype=torch.float64), steps=torch.tensor([0, 7, 9], dtype=torch.int32))
    ro = R.EnsembleRollout(torch.nn.Identity(), "cpu")
    with pytest.raises(RuntimeError):
        ro.state()
    got = ro.load_state(st).state()
    assert set(got) == {"T", "t", "t_end", "steps"}
    for k in st:
        assert got[k].dtype == st[k].dtype and torch.equal(got[k], st[k]), k
    got["T"].zero_()                                        # state() hands out copies
    assert torch.equal(ro.state()["T"], st["T"])
    ro2 = R.EnsembleRollout(torch.nn.Identity(), "cpu").load_state(got | dict(T=st["T"][:, 0]))    # [B,H,W] is accepted
    assert torch.equal(ro2.state()["T"], st["T"])
    with pytest.raises(ValueError):
        ro.load_state(dict(st, t=st["t"][:2]))
    with pytest.raises(RuntimeError):                       # no grid, no parameters: reset() comes first
        ro.run(1)


def test_cli_arguments():
    from pbml_mantle_convection_amd import rollout as R
    a = R.build_arg_parser().parse_args("--params p.csv --steps 3 --out o --synthetic 2 32 48 -l 2 -f 8 -r 2 -k 5 -p zeros".split())
    assert (a.levels, a.c_h, a.repeats, a.kernel, a.r_p, a.synthetic, a.steps) == (2, 8, 2, 5, "zeros", [2, 32, 48], 3)
    assert a.t_end is None and a.snapshot_every == 0 and a.weights is None

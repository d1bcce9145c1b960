"""CPU-only checks of the guarded optimizer step: argument validation of the two entry points (nothing is launched), the
workspace size function, the ctypes mirror of mc_grad_guard against the header, the two CLI flags, and build_model passing
`factor` to NewFluidNet."""
import ctypes as C
import math
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_EINVAL = -1
A = 0x10000          # an aligned address that is never dereferenced: validation fails before any launch


def _eval(grad=A, numel=8, scale=1.0, max_norm=0.0, skip=1, ws=A, guard=A, step=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_grad_guard_eval(grad, numel, scale, max_norm, skip, ws, guard, step, None)


def _adam(param=A, grad=A, m=A, v=A, numel=8, lr=A, step=A, guard=A):
    from pbml_mantle_convection_amd import _lib as L
    return L.load().mc_adam_step_flat_guarded(param, grad, m, v, numel, lr, 0.9, 0.999, 1e-8, 0.0, 1.0, step, guard, None)


def test_guard_entry_points_validate_arguments_without_gpu():
    from pbml_mantle_convection_amd import _lib as L
    assert L.load().mc_strerror(MC_EINVAL).startswith(b"invalid argument")
    for kw in (dict(grad=None), dict(ws=None), dict(guard=None), dict(step=None),          # null pointers
               dict(numel=0), dict(numel=-4),
               dict(grad=A + 4), dict(ws=A + 4), dict(guard=A + 2),                         # misaligned buffers
               dict(max_norm=-1.0), dict(max_norm=float("nan"))):
        assert _eval(**kw) == MC_EINVAL, kw
    for kw in (dict(param=None), dict(grad=None), dict(m=None), dict(v=None), dict(lr=None), dict(step=None), dict(guard=None),
               dict(numel=0),
               dict(param=A + 4), dict(grad=A + 8), dict(m=A + 4), dict(v=A + 12), dict(guard=A + 2)):
        assert _adam(**kw) == MC_EINVAL, kw
    import pytest
    with pytest.raises(L.MantleHipError):
        L.call("mc_grad_guard_eval", None, 8, 1.0, 0.0, 1, None, None, None, None)


def test_grad_norm_blocks():
    from pbml_mantle_convection_amd import _lib as L
    nb = lambda n: L.call("mc_grad_norm_blocks", n)  # noqa: E731
    assert nb(1) == 1 and nb(1024) == 1 and nb(0) == 0
    sizes = [1, 3, 4, 5, 255, 1023, 1024, 1025, 1028, 10007, 2048 * 256 * 4 + 5, 1 << 24, 29_000_000, 1 << 31, 1 << 40]
    vals = [nb(n) for n in sizes]
    assert all(a <= b for a, b in zip(vals, vals[1:])), vals
    assert nb(1028) == 2                                    # 257 float4 -> a second block
    assert vals[-1] == vals[-2] == nb(1 << 24) == 1024      # capped: the second launch takes four partials per lane


def test_grad_guard_mirror_matches_header():
    from pbml_mantle_convection_amd import _lib as L
    assert C.sizeof(L.GradGuard) == 32
    src = open(os.path.join(ROOT, "include", "mantle_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*mc_grad_guard;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"float": 4, "uint32_t": 4}
    off, want = 0, []
    for ty, name, arr in re.findall(r"(float|uint32_t)\s+(\w+)(?:\[(\d+)\])?;", body):
        want.append((name, off))
        off += size[ty] * int(arr or 1)
    assert off == 32
    assert want == [(n, getattr(L.GradGuard, n).offset) for n, _ in L.GradGuard._fields_]
    assert [n for n, _ in want] == ["norm", "coef", "nonfinite", "skip", "skipped", "consecutive", "pad"]


def test_cli_flags():
    from pbml_mantle_convection_amd import multigpu as G
    a = G.build_arg_parser().parse_args([])
    assert (a.clip_norm, a.skip_nonfinite) == (0.0, 0)
    a = G.build_arg_parser().parse_args("--clip_norm 1.5 --skip_nonfinite 1".split())
    assert (a.clip_norm, a.skip_nonfinite) == (1.5, 1)
    assert math.isclose(a.clip_norm, 1.5)


def test_build_model_passes_factor_to_newfluidnet():
    from pbml_mantle_convection_amd import multigpu as G
    from pbml_mantle_convection_amd.engine import PoolNode
    m = G.build_model("newfluidnet", 3, 7, 8, 3, torch.device("cpu"), "gelu", "zeros", "mae", True, 2, 5, p_pred=True, factor=3)
    pools = [n for n in m._graph.nodes if isinstance(n, PoolNode)]
    assert pools and any(n.f == 3 for n in pools), [n.f for n in pools]
    m2 = G.build_model("newfluidnet", 3, 7, 8, 3, torch.device("cpu"), "gelu", "zeros", "mae", True, 2, 5, p_pred=True)
    assert all(n.f != 3 for n in m2._graph.nodes if isinstance(n, PoolNode))

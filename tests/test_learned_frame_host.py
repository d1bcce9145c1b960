"""CPU-only checks of the learned-padding frame entry points (mc_learned_*): the ABI is declared, exported and bound; the
host-side validator refuses what the kernels could not index; and the frame's index map -- bank class and window origin
per output pixel, as include/mantle_hip.h states it -- is the nine rectangles of engine.learned_regions."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ("mc_learned_validate", "mc_learned_bank_bytes", "mc_learned_wgrad_workspace_bytes",
                "mc_learned_pack_banks_batched", "mc_learned_frame_fwd", "mc_learned_frame_dgrad", "mc_learned_frame_wgrad")

# (h, w, k, bc_x, bc_y) the validator must accept
ACCEPTED = [(6, 7, 5, 1, 1), (8, 31, 5, 1, 1), (8, 31, 5, 4, 1), (16, 16, 5, 2, 2), (3, 4, 3, 1, 1)]


def _desc(h, w, k, bc_x, bc_y, n=2, c_in=10, c_out=16, dtype=0, sym_h=4):
    from pbml_mantle_convection_amd import _lib as L
    return L.LearnedDesc(n, h, w, c_in, c_out, k, bc_x, bc_y, dtype, sym_h)


def test_frame_entry_points_declared_exported_and_bound():
    from pbml_mantle_convection_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "mantle_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mc_[a-z0-9_]+)\s*\(", src))
    lib = L.load()
    for name in ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in mantle_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    assert "mc_learned_desc" in src and C.sizeof(L.LearnedDesc) == 10 * 4
    assert C.sizeof(L.ConvDesc) == 15 * 4                       # mc_conv_desc is untouched
    assert len(L.LEARNED_FRAME_BANKS) == 8 and "conv" not in L.LEARNED_FRAME_BANKS


def test_validator_accepts_and_refuses_on_the_host():
    from pbml_mantle_convection_amd import _lib as L
    L.load()

    def check(d):
        return L.call("mc_learned_validate", C.byref(d))

    for dtype in (L.MC_F32, L.MC_BF16, L.MC_MIX16):
        for shp in ACCEPTED:
            d = _desc(*shp, dtype=dtype)
            assert check(d) == 0, shp
            assert L.call("mc_learned_bank_bytes", C.byref(d), 0) > 0 and L.call("mc_learned_bank_bytes", C.byref(d), 1) > 0
            assert L.call("mc_learned_wgrad_workspace_bytes", C.byref(d)) > 0
    assert check(_desc(5, 7, 5, 1, 1)) == -2                    # h < pad_y = 6
    assert check(_desc(8, 8, 5, 4, 1)) == -2                    # pad_x = 9 > w
    assert check(_desc(8, 5, 5, 1, 1)) == -2                    # w < pad_x
    assert check(_desc(16, 16, 4, 1, 1)) == -2                  # k = 4
    assert check(_desc(16, 16, 5, 1, 1, sym_h=3)) == -2         # odd number of mirrored filters
    assert check(_desc(16, 16, 5, 1, 1, dtype=7)) == -2         # unknown dtype
    assert check(_desc(2, 9, 3, 1, 1)) == -2                    # h < k
    bad = _desc(5, 7, 5, 1, 1)
    assert L.call("mc_learned_bank_bytes", C.byref(bad), 0) == 0 and L.call("mc_learned_wgrad_workspace_bytes", C.byref(bad)) == 0
    # every launch entry point validates first: a refused descriptor never reaches a launch (no device is touched here)
    lib = L.load()
    one = C.c_void_p(8)
    arr8 = (C.c_void_p * 8)(*[8] * 8)
    arr1 = (C.c_void_p * 1)(8)
    assert lib.mc_learned_frame_fwd(C.byref(bad), one, one, one, one, None) == -2
    assert lib.mc_learned_frame_dgrad(C.byref(bad), one, one, one, None) == -2
    assert lib.mc_learned_frame_wgrad(C.byref(bad), one, one, one, arr8, one, None) == -2
    assert lib.mc_learned_pack_banks_batched(C.byref(bad), arr8, arr1, arr1, 1, None) == -2
    assert lib.mc_learned_frame_fwd(C.byref(_desc(8, 31, 5, 1, 1)), None, None, None, None, None) == -1
    assert lib.mc_learned_validate(None) == -1


def frame_map(h, w, k, bc_x, bc_y):
    """The operator's index map, restated: {(oy, ox): (bank, iy0, ix0)} for every frame pixel, and the output size."""
    pad_x = k + 1 + (bc_x - 1) if k == 5 else k + (bc_x - 1)
    pad_y = k + 1 + (bc_y - 1) if k == 5 else k + (bc_y - 1)
    fx, fy, mh, mw = pad_x - k + 1, pad_y - k + 1, h - k + 1, w - k + 1
    ho, wo = mh + 2 * fy, mw + 2 * fx
    out = {}
    for oy in range(ho):
        for ox in range(wo):
            if oy < fy:
                row, iy0 = "bottom", h - pad_y + oy
            elif oy >= fy + mh:
                row, iy0 = "top", oy - (fy + mh)
            else:
                row, iy0 = "", oy - fy
            if ox < fx:
                col, ix0 = "left", ox
            elif ox >= fx + mw:
                col, ix0 = "right", w - pad_x + (ox - fx - mw)
            else:
                col, ix0 = "", ox - fx
            if row or col:
                out[(oy, ox)] = ("conv_" + "_".join(t for t in (row, col) if t), iy0, ix0)
    return ho, wo, out


@pytest.mark.parametrize("shape", ACCEPTED)
def test_frame_index_map_is_the_nine_rectangles(shape):
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd.engine import BANKS, learned_regions
    h, w, k, bc_x, bc_y = shape
    fy, fx, ho, wo, regs = learned_regions(h, w, k, bc_x, bc_y)
    mho, mwo, fmap = frame_map(h, w, k, bc_x, bc_y)
    assert (mho, mwo) == (ho, wo)
    assert set(regs) == set(BANKS) and set(L.LEARNED_FRAME_BANKS) == set(BANKS) - {"conv"}
    seen = {}
    for name, (sy, sx, sh, sw, dy, dx) in regs.items():
        assert sy >= 0 and sx >= 0 and sy + sh <= h and sx + sw <= w
        for r in range(sh - k + 1):
            for c in range(sw - k + 1):
                assert (dy + r, dx + c) not in seen, "the nine destination rectangles overlap"
                seen[(dy + r, dx + c)] = (name, sy + r, sx + c)
    assert len(seen) == ho * wo, "the nine destination rectangles do not tile the output"
    assert {p: v for p, v in seen.items() if v[0] != "conv"} == fmap
    # every window of the frame stays inside the input
    for name, iy0, ix0 in fmap.values():
        assert 0 <= iy0 and iy0 + k <= h and 0 <= ix0 and ix0 + k <= w


def test_single_layer_graph_carries_bc_and_input_gradient():
    from pbml_mantle_convection_amd import _lib as L
    from pbml_mantle_convection_amd import engine as E
    g = E.single_layer_graph(10, 16, 5, 2, "zeros", 4, L.POST_NONE, "gelu", 1, False, learned=True, bc_x=4, bc_y=1, input_grad=True)
    size, grad, convs = E.shape_walk(g, 2, 20, 141, "fp32")
    assert size[1] == (20 - 4 + 2 * 2, 141 - 4 + 2 * 5) and grad[0] and convs[0].dgrad
    assert len(list(E.iter_conv_descs(g, 2, 20, 141, "fp32"))) == 9       # the nine per-bank descriptors stay
    assert not E.shape_walk(E.single_layer_graph(10, 16, 5, 2, "zeros", 4, L.POST_NONE, "gelu", 1, False, learned=True),
                            2, 20, 141, "fp32")[1][0]

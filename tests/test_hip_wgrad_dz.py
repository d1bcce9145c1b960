"""The filter-gradient launch that forms dY from dz while it stages its tiles (mc_conv2d_wgrad_dz, MANTLE_WGRAD_DZ).

For a conv -> GroupNorm -> act layer whose dz = dA act'(z) comes from its consumer's input-gradient launch, the launch reads
(dz, z, a per-(sample, channel) coefficient table) instead of dY, evaluates mc_gn_bwd_apply_dz's expression with the same
operations in the same order, accumulates the filter gradient of the value it formed and stores it for the input-gradient
launch.  Nothing is re-associated, so every comparison here is bitwise: dY against mc_gn_bwd_apply_dz, the partial slabs and
(dW, db) against mc_conv2d_wgrad_fused on that dY, the coefficient table's m12 against the plain finalize kernels, and a
training step with the switch on against one with it off."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 4096                                     # bf16 elements in front of and behind the dY buffer
MC_EUNSUPPORTED = -2                             # include/mantle_hip.h


def _cb8(t, dtype):
    """NCHW f32 -> CB8 [N][C8][H][W][8] tensor of `dtype` on the device (padded channels zero)."""
    n, c, h, w = t.shape
    c8 = (c + 7) // 8
    o = torch.zeros((n, c8 * 8, h, w), dtype=torch.float32)
    o[:, :c] = t
    return o.view(n, c8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(DEV).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dz_values(shape, g):
    """bf16-representable dz with exact zeros of both signs and values on either side of the smallest normal bf16."""
    dz = torch.randn(shape, generator=g).bfloat16().float()
    flat = dz.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:96]
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 2.0 ** -127, -2.0 ** -128, 2.0 ** -125, 2.0 ** -133])
    flat[idx] = special.repeat(12)
    return dz


def _case(H, W, ci, co, kind, seed):
    """Runs both chains on one set of operands and returns everything the assertions need."""
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    N, k, p, groups = 2, 5, 2, 4
    mode = L.PAD_MODES["reflect"]
    g = torch.Generator().manual_seed(seed)
    st = torch.cuda.current_stream().cuda_stream
    cop = (co + 7) // 8 * 8
    x = _cb8(torch.randn((N, ci, H, W), generator=g), torch.float16)
    z = _cb8(torch.randn((N, co, H, W), generator=g) * 3.0, torch.float16)
    dzv = _dz_values((N, co, H, W), g)
    dz = _cb8(dzv, torch.bfloat16)
    if kind == "padfold":
        # the padded-domain buffer of the consumer's input gradient: the frame holds junk that is not the interior's
        buf = torch.full((N, cop // 8, H + 2 * p, W + 2 * p, 8), 777.0, dtype=torch.bfloat16, device=DEV)
        buf[:, :, p:p + H, p:p + W] = dz
        gs = L.GradSrc(buf.data_ptr(), L.GSRC_PADFOLD, p, mode, 1, H, W, 0, 0)
    else:
        buf = dz
        gs = L.GradSrc(buf.data_ptr(), L.GSRC_PLAIN, 0, 0, 1, H, W, 0, 0)
    # the layer's (scale, shift, mean, rstd) table as mc_gn_finalize_coef forms it; padded channels zero
    cpg = co // groups
    mean = 0.2 + 0.1 * torch.randn((N, groups), generator=g)
    rstd = 0.8 + 0.1 * torch.rand((N, groups), generator=g)
    gamma, beta = 1 + 0.2 * torch.randn(co, generator=g), 0.1 * torch.randn(co, generator=g)
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    coef = torch.zeros((N, cop, 4))
    coef[:, :co] = torch.stack([rstd_c * gamma, beta - mean_c * rstd_c * gamma, mean_c, rstd_c], -1)
    coef, gamma = coef.to(DEV), gamma.to(DEV)
    # partial sums of the reduction (any values: the finalize kernels only add them up)
    blocks = 300 if cpg == 4 and H > 20 else 7        # > 256 slots: the per-(group, sample) finalize, as the engine chooses
    part = torch.randn((N, blocks, cop, 2), generator=g).to(DEV)
    d = L.ConvDesc(N, H, W, ci, 0, co, k, p, mode, L.MC_MIX16, 0, 0, 0)

    def finalize(with_table):
        m12 = torch.zeros((N, groups, 2), device=DEV)
        dg, db_ = torch.zeros(co, device=DEV), torch.zeros(co, device=DEV)
        pc = torch.zeros((N, cop, 2), device=DEV)
        tab = torch.zeros((N, cop, 4), device=DEV)
        extra = (coef.data_ptr(), tab.data_ptr()) if with_table else ()
        sfx = "_dz" if with_table else ""
        if blocks > 256:
            L.call("mc_gn_act_bwd_finalize_n" + sfx, part.data_ptr(), N, blocks, co, groups, H * W, gamma.data_ptr(), m12.data_ptr(),
                   pc.data_ptr(), *extra, st)
        else:
            L.call("mc_gn_act_bwd_finalize" + sfx, part.data_ptr(), N, blocks, co, groups, H * W, gamma.data_ptr(), m12.data_ptr(),
                   dg.data_ptr(), db_.data_ptr(), *extra, st)
        return m12, dg, db_, pc, tab

    ref_fin, new_fin = finalize(False), finalize(True)
    m12, tab = ref_fin[0], new_fin[4]

    def dy_buffer():
        raw = torch.full((2 * GUARD + N * cop * H * W,), 123.0, dtype=torch.bfloat16, device=DEV)
        return raw, raw[GUARD:GUARD + N * cop * H * W].view(N, cop // 8, H, W, 8)

    def weight_grads(wpart):
        dw, db_ = torch.zeros((co, ci, k, k), device=DEV), torch.zeros(co, device=DEV)
        descs = (L.ConvDesc * 1)(d)
        L.call("mc_conv2d_wgrad_finalize_batched", descs, (C.c_void_p * 1)(wpart.data_ptr()), (C.c_void_p * 1)(dw.data_ptr()),
               (C.c_void_p * 1)(db_.data_ptr()), 1, st)
        return dw, db_

    nbytes = lib.mc_wgrad_partial_bytes(C.byref(d))
    # the present chain: apply pass, then the filter gradient of its dY
    raw_a, dy_a = dy_buffer()
    L.call("mc_gn_bwd_apply_dz", C.byref(gs), z.data_ptr(), N, co, H, W, groups, coef.data_ptr(), m12.data_ptr(), L.MC_MIX16,
           dy_a.data_ptr(), st)
    wp_a = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    L.call("mc_conv2d_wgrad_fused", C.byref(d), x.data_ptr(), None, None, dy_a.data_ptr(), wp_a.data_ptr(), st)
    # the new launch
    raw_b, dy_b = dy_buffer()
    wp_b = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    L.call("mc_conv2d_wgrad_dz", C.byref(d), x.data_ptr(), None, C.byref(gs), z.data_ptr(), tab.data_ptr(), dy_b.data_ptr(),
           wp_b.data_ptr(), st)
    ga, gb = weight_grads(wp_a), weight_grads(wp_b)
    torch.cuda.synchronize()
    return dict(ref_fin=ref_fin, new_fin=new_fin, raw_a=raw_a, raw_b=raw_b, dy_a=dy_a, dy_b=dy_b, wp_a=wp_a, wp_b=wp_b, ga=ga, gb=gb,
                coef=coef, N=N, co=co, cop=cop, groups=groups)


# 16x32: one exact tile; 17x33: a one-pixel ragged row and column; 20x40: 2 x 2 tiles, both edges ragged; 36x70: interior and
# edge tiles; 10 -> 16 (padded input channels), 16 -> 16, and a partly filled output block (12).  The grid has one block per
# work item up to 768 blocks, so "several work items per block" (a block forms a second tile while the first one's loads are
# behind it) needs more than 768 tiles: 309x647 is 2 x 20 x 21 = 840, ragged on both edges.
SHAPES = [(16, 32, 16, 16), (17, 33, 16, 16), (20, 40, 10, 16), (36, 70, 16, 16), (36, 70, 10, 16), (20, 40, 16, 12),
          (309, 647, 16, 16)]


@pytest.mark.parametrize("kind", ["padfold", "plain"])
@pytest.mark.parametrize("H,W,ci,co", SHAPES)
def test_wgrad_dz_equals_apply_then_filter_gradient(H, W, ci, co, kind):
    r = _case(H, W, ci, co, kind, seed=H * 1000 + W * 10 + ci + co)
    # the coefficient-writing finalize forms leave everything the plain forms leave
    for a, b, what in zip(r["ref_fin"][:4], r["new_fin"][:4], ("m12", "dgamma", "dbeta", "chan_sums")):
        assert _same(a, b), what
    # ... and the table: rows of real channels are finite and carry the layer's mean, padded rows stay zero
    tab = r["new_fin"][4]
    assert torch.isfinite(tab).all()
    assert _same(tab[:, :co, 3], r["coef"][:, :co, 2]) and _same(tab[:, :co, 0], r["coef"][:, :co, 0])
    assert not tab[:, co:].any()
    # dY: the apply pass's, bit for bit, and nothing outside the tensor is written
    assert _same(r["dy_b"], r["dy_a"]), int((_bits(r["dy_b"]) != _bits(r["dy_a"])).sum())
    assert float(r["dy_a"].float().abs().max()) > 0.1                    # (the comparison is not between two empty buffers)
    for raw in (r["raw_a"], r["raw_b"]):
        assert bool((raw[:GUARD] == 123.0).all()) and bool((raw[-GUARD:] == 123.0).all())
    # filter gradient: the same slabs, the same (dW, db)
    assert torch.equal(r["wp_b"], r["wp_a"])
    assert _same(r["gb"][0], r["ga"][0]) and _same(r["gb"][1], r["ga"][1])
    assert float(r["ga"][0].abs().max()) > 0 and float(r["ga"][1].abs().max()) > 0


@pytest.mark.parametrize("ci,co,dt", [(32, 16, "mixed"), (16, 32, "mixed"), (16, 16, "bf16"), (16, 16, "fp32")])
def test_wgrad_dz_refuses_what_it_does_not_cover(ci, co, dt):
    """Two input-channel chunks, two output-channel groups, the plain bf16 and fp32 modes: MC_EUNSUPPORTED, nothing launched
    (dY and the partial slabs keep their fill)."""
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    N, H, W, k, p = 2, 20, 40, 5, 2
    mcd, xdt, gdt = {"mixed": (L.MC_MIX16, torch.float16, torch.bfloat16), "bf16": (L.MC_BF16, torch.bfloat16, torch.bfloat16),
                     "fp32": (L.MC_F32, torch.float32, torch.float32)}[dt]
    g = torch.Generator().manual_seed(5)
    x = _cb8(torch.randn((N, ci, H, W), generator=g), xdt)
    z = _cb8(torch.randn((N, co, H, W), generator=g), xdt)
    dz = _cb8(torch.randn((N, co, H, W), generator=g), gdt)
    tab = torch.zeros((N, (co + 7) // 8 * 8, 4), device=DEV)
    dy = torch.full((N, (co + 7) // 8, H, W, 8), 5.0, dtype=gdt, device=DEV)
    d = L.ConvDesc(N, H, W, ci, 0, co, k, p, L.PAD_MODES["reflect"], mcd, 0, 0, 0)
    wp = torch.full((lib.mc_wgrad_partial_bytes(C.byref(d)),), 7, dtype=torch.uint8, device=DEV)
    gs = L.GradSrc(dz.data_ptr(), L.GSRC_PLAIN, 0, 0, 1, H, W, 0, 0)
    rc = lib.mc_conv2d_wgrad_dz(C.byref(d), x.data_ptr(), None, C.byref(gs), z.data_ptr(), tab.data_ptr(), dy.data_ptr(),
                                wp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == MC_EUNSUPPORTED, rc
    assert bool((dy == 5.0).all()) and bool((wp == 7).all())


def test_wgrad_dz_refuses_a_dz_of_another_shape():
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    N, H, W = 2, 20, 40
    x = torch.zeros((N, 2, H, W, 8), dtype=torch.float16, device=DEV)
    dz = torch.zeros((N, 2, H, W, 8), dtype=torch.bfloat16, device=DEV)
    tab = torch.zeros((N, 16, 4), device=DEV)
    dy = torch.full((N, 2, H, W, 8), 5.0, dtype=torch.bfloat16, device=DEV)
    d = L.ConvDesc(N, H, W, 16, 0, 16, 5, 2, L.PAD_MODES["reflect"], L.MC_MIX16, 0, 0, 0)
    wp = torch.full((lib.mc_wgrad_partial_bytes(C.byref(d)),), 7, dtype=torch.uint8, device=DEV)
    gs = L.GradSrc(dz.data_ptr(), L.GSRC_PLAIN, 0, 0, 1, H - 1, W, 0, 0)
    rc = lib.mc_conv2d_wgrad_dz(C.byref(d), x.data_ptr(), None, C.byref(gs), x.data_ptr(), tab.data_ptr(), dy.data_ptr(),
                                wp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == MC_EUNSUPPORTED, rc
    assert bool((dy == 5.0).all()) and bool((wp == 7).all())


# ------------------------------------------------------------------------------------------------------------------
# network level: one training step with the switch on and one with it off, each in a fresh process
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    out = {}
    for sw in ("1", "0"):
        path = str(tmp_path_factory.mktemp("wgrad_dz") / f"sw{sw}.npz")
        env = dict(os.environ, MANTLE_WGRAD_DZ=sw, HIP_VISIBLE_DEVICES="0")
        env.pop("MANTLE_FUSE", None)
        r = subprocess.run([sys.executable, os.path.join(HERE, "wgrad_dz_worker.py"), path], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        out[sw] = np.load(path, allow_pickle=False)
    return out


# the issue's case (40 x 48: the dz epilogue, and so the new launch, run with MANTLE_FUSE=2 only), the same with that setting,
# and a grid wide enough for the default execution to take the new launch
@pytest.mark.parametrize("cfg,active", [("narrow", False), ("narrow_fuse2", True), ("wide", True)])
def test_training_step_is_bit_identical_with_and_without_the_switch(steps, cfg, active):
    on, off = steps["1"], steps["0"]
    assert (int(on[cfg + "_layers"]) > 0) == active, int(on[cfg + "_layers"])      # layers whose dY the new launch forms
    assert int(off[cfg + "_layers"]) == 0
    for what in ("grad", "param"):
        a, b = on[f"{cfg}_eager_{what}"], off[f"{cfg}_eager_{what}"]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (cfg, what, float(np.abs(a - b).max()))
        assert np.isfinite(a).all() and np.abs(a).max() > 0
    # switch on: the captured step equals the eager one, and two replays of the captured chain equal each other
    for sw in (on, off):
        for what in ("grad", "param"):
            assert np.array_equal(sw[f"{cfg}_graph_{what}"].view(np.int32), sw[f"{cfg}_eager_{what}"].view(np.int32)), (cfg, what)
        assert np.array_equal(sw[f"{cfg}_replay1"].view(np.int32), sw[f"{cfg}_replay2"].view(np.int32)), cfg

"""Every convolution kernel variant against f64, straight through the C ABI, at the smallest shapes at which its index
arithmetic can go wrong (tests/conv_variants.py: the case table, pinned to the dispatch by kernel name, the f64 references
and the derived per-element tolerance).

  test_case_table_reaches_every_kernel_variant   host only: each case reaches the instantiation written next to it
  test_comparison_rejects_wrong_padding_and_unflipped_filters   CPU only: the comparison has teeth
  test_forward / test_input_gradient / test_filter_gradient     GPU: one launch each per (case, precision)

The GPU tests place every buffer a launch writes between two sentinel bands (at least one tile row of the tensor) and check
them afterwards, prefill outputs with NaN, and surround the inputs with garbage instead of zeros.

Every test prints its worst err / tol (`pytest -s`).  On MI355X, worst case per kernel family (MC_BF16 / MC_MIX16):
  k_conv_direct_f32   y 0.021 (f32-k3-2tile-1), input gradient 0.024, GroupNorm sums 0.001
  k_conv_mfma_bf16    y 0.990 / 0.955 (w3-nt4-2tile-1), input gradient 0.993 (w3-nt1-f32out), GroupNorm sums 0.001
  k_conv_rr_bf16      y 0.993 / 0.975 (rr3-persistent), input gradient 0.977 (rr3-dgrad-w141), GroupNorm sums 0.001
  filter gradient     dw 0.070 (f32), 0.062 / 0.062 (w5-8r-nt2-min-reflect); dbias 0.011 (f32), < 0.001 (16-bit)
A 16-bit output sits just under 1 by construction: its error is the final rounding, at worst u |ref| of the u (|ref| + E) + E
allowed.  The sums' bound adds every pixel's worst case and is therefore loose: a missing, doubled or misplaced tile is far
outside it, a difference in the last bits is not."""
import ctypes as C

import pytest
import torch

import conv_variants as V
from oracle import ref_cpu as O
from pbml_mantle_convection_amd import _lib as L

DEV = "cuda:0"
SENTINEL = 0x7B           # as bf16 / f32 1.3e36, as f16 61280: garbage that shows in any result it leaks into
CB8 = 8


# ---- host only ----------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_kernel_variant():
    """mc_conv_kernel_name needs no device: every forward and every input-gradient descriptor of the table reaches the kernel
    written next to it, MC_MIX16 takes the instantiation MC_BF16 takes (the name does not carry the element type), and the
    table as a whole reaches exactly the written list."""
    reached = set()
    for cid, dt in V.RUNS:
        c = V.CASE_BY_ID[cid]
        d, dd = V.descs(c, dt)
        assert V.kernel_name(d) == c.fwd, (cid, dt, "forward", V.kernel_name(d))
        assert V.kernel_name(dd) == c.dgrad, (cid, dt, "input gradient", V.kernel_name(dd))
        reached |= {c.fwd, c.dgrad}
    assert reached == V.KERNELS, reached ^ V.KERNELS


def test_case_table_follows_the_shape_rules():
    """The rules the table was built by, so that a later edit keeps them: sample stride, padded / one / three K-chunks, both
    concat splits, ragged output channels, all padding modes, mirrored filters, outputs of tile + 1, 2 tile - 1 and less than a
    tile in both axes, the row-reuse widths and the persistent loops (N x tiles above the work-group cap of rr_launch /
    mc_conv2d_bf16)."""
    sixteen = [c for c in V.CASES if not c.f32]
    assert all(c.n >= 2 for c in V.CASES)
    for fam in ("k_conv_direct_f32", "k_conv_mfma_bf16", "k_conv_rr_bf16"):
        cs = [c for c in V.CASES if c.fwd.startswith(fam)]
        assert {sum(c.ci) for c in cs} >= {11, 16, 48}, fam
        assert {c.mode for c in cs} == {"zeros", "replicate", "reflect"}, fam
        assert any(c.sym[0] > 0 for c in cs), fam
        assert any(c.co % 8 for c in cs), fam
        assert any(c.k == 5 and c.mode == "reflect" and c.hw == (3, 3) for c in cs), fam
        rel = [(V.out_hw(c), V.tile_of(c.fwd)) for c in cs]       # output size against the tile of the case's own kernel
        assert any(o == (th + 1, tw + 1) for o, (th, tw) in rel), fam
        assert any(o == (2 * th - 1, 2 * tw - 1) for o, (th, tw) in rel), fam
        assert any(o[0] < th and o[1] < tw for o, (th, tw) in rel), fam
    assert {c.ci for c in V.CASES if len(c.ci) == 2} == {(16, 8), (8, 12)}
    assert {c.co for c in V.CASES if c.co % 8} == {4, 20}
    assert any(c.sym[1] > 0 and c.sym[2] > 0 for c in sixteen)
    assert {c.hw[1] for c in V.CASES if c.fwd.startswith("k_conv_rr_bf16")} >= {63, 65, 129}
    lib = L.load()
    for cid, groups, cap in (("rr3-persistent", 3, 256), ("w5-persistent", 3, 4096)):
        c = V.CASE_BY_ID[cid]
        d, _ = V.descs(c, "bf16")
        tiles = lib.mc_conv_tiles(C.byref(d)) // (4 if cid.startswith("rr") else 1)      # (row reuse: one slot per strip)
        assert c.n * tiles > cap // groups, (cid, c.n * tiles, cap // groups)


# ---- CPU only: the comparison has teeth -----------------------------------------------------------------------------------
WRONG_MODE = {"reflect": "replicate", "replicate": "zeros", "zeros": "replicate"}


@pytest.mark.parametrize("cid,dt", V.RUNS, ids=V.RUN_IDS)
def test_comparison_rejects_wrong_padding_and_unflipped_filters(cid, dt):
    """The forward reference evaluated with another padding mode, and with the mirrored filters left unflipped, rounded to the
    stored type like a kernel's output, must FAIL the comparison the GPU tests use; the failures of the padding mutant lie
    within `pad` of the border (everywhere else the mutant is the reference, and passes)."""
    c = V.CASE_BY_ID[cid]
    r = V.forward_ref(cid, dt)
    x, wu, b, _ = V.inputs(cid)
    ft = V.FWD_T[dt]
    x64, w64, b64 = V.rnd(x, ft), V.rnd(wu, ft), b.double()
    stored = lambda t: t.to(torch.float32).to(r.store).double()      # noqa: E731
    assert not V.compare(stored(r.y), r.y, r.tol)[1].any()           # (the reference itself passes)
    hole = stored(r.y)
    hole[-1, -1, -1, -1] = float("nan")                              # (an element the kernel never wrote: the NaN prefill)
    assert int(V.compare(hole, r.y, r.tol)[1].sum()) == 1
    p = V.pad_of(c)
    mutant = V.forward_eval(c, x64, O.expand_symmetric_weight(w64, V.sym_dict(c)), b64, mode=WRONG_MODE[c.mode])
    bad = V.compare(stored(mutant), r.y, r.tol)[1]
    assert bad.any(), "padding mutant passes: the inputs are too tame"
    assert not bad[:, :, p:bad.shape[2] - p, p:bad.shape[3] - p].any()
    if any(c.sym):
        mutant = V.forward_eval(c, x64, V.expand_unflipped(w64, c), b64)
        bad = V.compare(stored(mutant), r.y, r.tol)[1]
        nu = wu.shape[0]
        assert bad[:, nu:].any() and not bad[:, :nu].any(), "unflipped-filter mutant passes: the inputs are too tame"


# ---- GPU ----------------------------------------------------------------------------------------------------------------
class Guarded:
    """A tensor between two sentinel bands inside one larger allocation."""

    def __init__(self, shape, dtype, guard_bytes, fill=None):
        n = 1
        for s in shape:
            n *= int(s)
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        if fill is not None:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def assert_intact(self, what):
        lo, hi = self.raw[:self.g], self.raw[self.g + self.nbytes:]
        assert bool((lo == SENTINEL).all()), f"{what}: bytes BEFORE the buffer were overwritten"
        assert bool((hi == SENTINEL).all()), f"{what}: bytes BEHIND the buffer were overwritten"


def band(w, itemsize=4):
    """Sentinel bytes per side of a CB8 tensor of width w: 24 rows (the tallest tile) of one channel block."""
    return 24 * w * CB8 * itemsize


def pack(x, dtype_mc, tdt):
    """NCHW f32 (CPU) -> CB8 on the device through mc_pack_nchw, surrounded by garbage."""
    n, c, h, w = x.shape
    xd = x.to(DEV).contiguous()
    out = Guarded((n, (c + 7) // 8, h, w, CB8), tdt, band(w), fill=float("nan"))
    L.call("mc_pack_nchw", L.ptr(xd), n, c, c, h, w, 0, 0, None, dtype_mc, out.ptr, L.stream())
    return out


def unpack(buf, c, dtype_mc):
    n, _, h, w, _ = buf.t.shape
    r = torch.empty((n, c, h, w), dtype=torch.float32, device=DEV)
    L.call("mc_unpack_nchw", buf.ptr, n, c, h, w, 0, None, dtype_mc, L.ptr(r), L.stream())
    return r.cpu()


def lanes(buf):
    """CB8 [n][c8][h][w][8] -> [n][c8 * 8][h][w], every lane (the padded channels included)."""
    n, c8, h, w, _ = buf.t.shape
    return buf.t.permute(0, 1, 4, 2, 3).reshape(n, c8 * CB8, h, w).float().cpu()


def sources(c, dt):
    x = V.inputs(c.id)[0]
    ci0 = c.ci[0]
    x0 = pack(x[:, :ci0], V.MC[dt], V.FWD_T[dt])
    x1 = pack(x[:, ci0:], V.MC[dt], V.FWD_T[dt]) if len(c.ci) > 1 else None
    return x0, x1


def bank(c, d, dgrad):
    wu = V.inputs(c.id)[1].to(DEV).contiguous()
    nbytes = L.call("mc_packed_weight_bytes", C.byref(d), dgrad)
    assert nbytes > 0
    b = Guarded((nbytes,), torch.uint8, 65536)
    L.call("mc_pack_weights", C.byref(d), L.ptr(wu), dgrad, b.ptr, L.stream())
    torch.cuda.synchronize()
    b.assert_intact("filter bank")
    return b


def report(c, dt, kernel, **ratios):
    print(f"\n[{c.id} {dt}] {kernel}: worst err/tol " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def assert_within(what, got, ref, tol):
    ratio, bad = V.compare(got, ref, tol)
    if bad.any():
        idx = [tuple(int(v) for v in i) for i in bad.nonzero()[:8]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, worst err/tol {ratio:.3f}, "
                             f"first at {idx}")
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dt", V.RUNS, ids=V.RUN_IDS)
def test_forward(cid, dt):
    """y and stat_partials of the forward launch.  y against conv2d_same / expand_symmetric_weight in f64 on operands rounded
    as the kernel reads them; the lanes past c_out exactly zero; the per-tile (sum, sum of squares) added over the tiles
    against the f64 sums of the unrounded reference (V.stats_ref: the sums come from the f32 accumulators)."""
    L.load()
    c = V.CASE_BY_ID[cid]
    d, _ = V.descs(c, dt)
    ref = V.forward_ref(cid, dt)
    sref, stol = V.stats_ref(cid, dt)
    x0, x1 = sources(c, dt)
    bk = bank(c, d, 0)
    bias = V.inputs(cid)[2].to(DEV).contiguous()
    ho, wo = V.out_hw(c)
    c8 = (c.co + 7) // 8
    y = Guarded((c.n, c8, ho, wo, CB8), ref.store, band(wo), fill=float("nan"))
    slots = L.call("mc_conv_tiles", C.byref(d))
    part = Guarded((c.n, slots, c8 * CB8, 2), torch.float32, 65536, fill=float("nan"))
    L.call("mc_conv2d", C.byref(d), x0.ptr, x1.ptr if x1 else None, bk.ptr, L.ptr(bias), y.ptr, None, part.ptr, L.stream())
    torch.cuda.synchronize()
    for buf, what in ((y, "y"), (part, "stat_partials"), (x0, "x0"), (x1, "x1"), (bk, "filter bank")):
        if buf is not None:
            buf.assert_intact(what)
    got = unpack(y, c.co, L.MC_F32 if c.out_f32 else V.MC[dt])
    r_y = assert_within("y", got, ref.y, ref.tol)
    full = lanes(y)
    assert torch.equal(full[:, :c.co], got), "mc_unpack_nchw disagrees with the CB8 lanes"
    assert bool((full[:, c.co:] == 0).all()), "lanes past c_out are not zero"
    p = part.t.double().cpu()
    assert bool((p[:, :, c.co:] == 0).all()), "stat_partials of the padded channels are not zero"
    sums = p.sum(1)[:, :c.co]
    r_s1 = assert_within("sum y", sums[..., 0], sref[..., 0], stol[..., 0])
    r_s2 = assert_within("sum y^2", sums[..., 1], sref[..., 1], stol[..., 1])
    report(c, dt, c.fwd, y=r_y, sum=r_s1, sumsq=r_s2)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dt", V.RUNS, ids=V.RUN_IDS)
def test_input_gradient(cid, dt):
    """mc_conv2d on the input-gradient descriptor (padded domain, rotated / transposed bank, split outputs) against
    conv_transpose2d in f64.  The lanes past the channel count of either output are exactly zero."""
    L.load()
    c = V.CASE_BY_ID[cid]
    d, dd = V.descs(c, dt)
    ref, tol = V.dgrad_ref(cid, dt)
    mcg, gt = dd.dtype, V.GRAD_T[dt]
    dy = pack(V.inputs(cid)[3], mcg, gt)
    bk = bank(c, d, 1)
    hp, wp = ref.shape[2:]
    outs = [Guarded((c.n, (ci + 7) // 8, hp, wp, CB8), gt, band(wp), fill=float("nan")) for ci in c.ci]
    L.call("mc_conv2d", C.byref(dd), dy.ptr, None, bk.ptr, None, outs[0].ptr, outs[1].ptr if len(outs) > 1 else None, None,
           L.stream())
    torch.cuda.synchronize()
    for buf, what in ((outs[0], "dx0"), (outs[-1], "dx1"), (dy, "dy"), (bk, "filter bank")):
        buf.assert_intact(what)
    got = torch.cat([unpack(o, ci, mcg) for o, ci in zip(outs, c.ci)], 1)
    assert got.shape == ref.shape
    ratio = assert_within("dx", got, ref, tol)
    for o, ci in zip(outs, c.ci):
        assert bool((lanes(o)[:, ci:] == 0).all()), "lanes past the channel count are not zero"
    report(c, dt, c.dgrad, dx=ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,dt", V.RUNS, ids=V.RUN_IDS)
def test_filter_gradient(cid, dt):
    """mc_conv2d_wgrad into a workspace of exactly mc_wgrad_partial_bytes (prefilled with NaN: every slab the reduction reads
    must have been written), then mc_conv2d_wgrad_finalize, which ACCUMULATES, into buffers prefilled with 0.25; against f64
    autograd."""
    L.load()
    c = V.CASE_BY_ID[cid]
    d, dd = V.descs(c, dt)
    dw_ref, dw_tol, db_ref, db_tol = V.wgrad_ref(cid, dt)
    x0, x1 = sources(c, dt)
    dy = pack(V.inputs(cid)[3], dd.dtype, V.GRAD_T[dt])
    nbytes = L.call("mc_wgrad_partial_bytes", C.byref(d))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = Guarded((nbytes // 4,), torch.float32, 65536, fill=float("nan"))
    dw = Guarded(tuple(dw_ref.shape), torch.float32, 65536, fill=V.WGRAD_PREFILL)
    db = Guarded(tuple(db_ref.shape), torch.float32, 65536, fill=V.WGRAD_PREFILL)
    L.call("mc_conv2d_wgrad", C.byref(d), x0.ptr, x1.ptr if x1 else None, dy.ptr, ws.ptr, L.stream())
    torch.cuda.synchronize()
    for buf, what in ((ws, "filter-gradient workspace"), (x0, "x0"), (x1, "x1"), (dy, "dy")):
        if buf is not None:
            buf.assert_intact(what)
    L.call("mc_conv2d_wgrad_finalize", C.byref(d), ws.ptr, dw.ptr, db.ptr, L.stream())
    torch.cuda.synchronize()
    for buf, what in ((ws, "filter-gradient workspace"), (dw, "dw"), (db, "dbias")):
        buf.assert_intact(what)
    r_w = assert_within("dw", dw.t.cpu(), dw_ref, dw_tol)
    r_b = assert_within("dbias", db.t.cpu(), db_ref, db_tol)
    report(c, dt, "k_wgrad_mfma_bf16" if dt != "f32" else "k_wgrad_f32", dw=r_w, dbias=r_b)

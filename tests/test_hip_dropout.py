"""The dropout variants of the GroupNorm / activation kernels, straight through the C ABI.

At p = 0.5 the threshold is 32768 and the scale 2, exact in every storage type, so everything is EQUALITY: the forward is
2 m a0 with a0 the plain entry point's output, and every backward entry point given the sources g equals its plain twin given
2 m g prepared on the host (the build has -ffp-contract=off; both kernels then do the same f32 operations in the same order).
One exception, by the format and not by the kernel: where the stored a0 is an f16 SUBNORMAL (|a0| < 2^-14: GELU of a large
negative argument), rounding does not commute with doubling -- rnd(2 a) may be an odd multiple of 2^-24, 2 rnd(a) never is
-- so there, and only there, the two may differ by one subnormal step, 2^-24.
At p = 0.1 the dropped set must be the restatement's (tests/dropout_ref.py) and the kept values s a0 within the two store
roundings.  Outputs are prefilled with NaN and sit between sentinel bands."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dropout_ref as R
from pbml_mantle_convection_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7B
SEED, STEP, LAYER = (0x9E3779B9, 0x7F4A7C15), 5, 3
ACT, EPS = L.ACTS["gelu"], 1e-5

#        N, c, groups, H, W
CASES = [(2, 3, 1, 8, 8),          # 3 channels per group: generic kernels only
         (2, 8, 2, 9, 11),         # small and generic
         (3, 12, 3, 16, 63),       # ragged channel block: padded lanes
         (2, 6, 1, 40, 54),        # 6 channels per group
         (2, 16, 4, 70, 300)]      # 84 000 vectors, ragged 8-row blocks, several blocks; generic only
IDS = ["x".join(map(str, c)) for c in CASES]
DT = {"fp32": (L.MC_F32, torch.float32, torch.float32, 0.0), "bf16": (L.MC_BF16, torch.bfloat16, torch.bfloat16, 2.0 ** -8),
      "mixed": (L.MC_MIX16, torch.float16, torch.bfloat16, 2.0 ** -11)}


def small_ok(case):
    _, c, g, h, w = case
    return (c // g) in (1, 2, 4, 8) and h * w <= 64 * 64


class Guarded:
    """A tensor between two sentinel bands inside one larger allocation."""

    def __init__(self, shape, dtype, guard_bytes=65536, fill=float("nan")):
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.g = (int(guard_bytes) + 255) // 256 * 256
        self.raw = torch.full((2 * self.g + self.nbytes,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.t = self.raw[self.g:self.g + self.nbytes].view(dtype).view(*shape)
        if fill is not None:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.g] == SENTINEL).all()) and bool((self.raw[self.g + self.nbytes:] == SENTINEL).all())


def state(step=STEP):
    host = np.array([SEED[0], SEED[1], step, 0], dtype=np.uint32)
    return torch.from_numpy(host.view(np.int32).copy()).to(DEV)


def same(a, b):
    """Equal as numbers (signed zeros compare equal, a NaN never does)."""
    return bool((a.float() == b.float()).all())


def twice_masked(ad, a0, m2):
    """ad == 2 m a0 as numbers; f16 only: one subnormal step (2^-24) apart at most where a0 itself is subnormal."""
    want = a0.float() * m2
    diff = (ad.float() - want).abs()                # (NaN where ad is NaN: fails both comparisons below)
    ok = diff == 0
    if a0.dtype == torch.float16:
        ok |= (a0.float().abs() < 2.0 ** -14) & (diff <= 2.0 ** -24)
    return bool(ok.all())


@functools.lru_cache(maxsize=None)
def mask_cb8(case, p):
    n, c, _, h, w = case
    c8 = (c + 7) // 8
    return torch.from_numpy(R.keep_vectors(SEED, STEP, LAYER, 0, n * c8 * h * w, R.keep16(p)).reshape(n, c8, h, w, 8))


@functools.lru_cache(maxsize=None)
def host_inputs(case):
    n, c, groups, h, w = case
    gen = torch.Generator().manual_seed(1000 + 7 * c + h)
    # bounded: after GroupNorm |z| stays below ~4, where f32 GELU is never exactly zero (0.5 z (1 + erff(z / sqrt 2)) is -0
    # from z = -5.6 down, which 672 000 normal draws times gamma do reach) -- the p = 0.1 test reads the dropped set off zeros
    y = (torch.rand((n, c, h, w), generator=gen) * 2.0 - 1.0) * 1.5 + 0.3
    gamma = 1.0 + 0.3 * torch.randn(c, generator=gen)
    beta = 0.2 * torch.randn(c, generator=gen)
    grads = [torch.randn((n, c, h + 2 * pad, w + 2 * pad), generator=gen) for pad in (0, 2, 1)]
    return y, gamma, beta, grads


class Setup:
    """Device tensors of one (case, precision): y in CB8 with its GroupNorm statistics, and the gradient tensors."""

    def __init__(self, case, prec):
        self.case, (self.mc, self.tdt, self.gdt, self.u) = case, DT[prec]
        self.mcg = L.MC_BF16 if self.mc == L.MC_MIX16 else self.mc
        n, c, groups, h, w = case
        self.c8 = (c + 7) // 8
        y, gamma, beta, grads = host_inputs(case)
        self.gamma, self.beta = gamma.to(DEV), beta.to(DEV)
        self.st = L.stream()
        self.y = self.cb8(y, self.mc, self.tdt)
        self.tiles = min(64, h)
        self.part = torch.empty((n, self.tiles, self.c8 * 8, 2), dtype=torch.float32, device=DEV)
        self.stats = torch.empty((n, groups, 2), dtype=torch.float32, device=DEV)
        L.call("mc_gn_partials", L.ptr(self.y), n, c, h, w, self.mc, self.tiles, L.ptr(self.part), self.st)
        L.call("mc_gn_finalize", L.ptr(self.part), n, self.tiles, c, groups, h * w, EPS, L.ptr(self.stats), None, self.st)
        self.grads = [self.cb8(g, self.mcg, self.gdt) for g in grads]      # plain, pad 2, pad 1; lanes past c are zero

    def cb8(self, x, mc, tdt):
        n, c, h, w = x.shape
        out = torch.zeros((n, (c + 7) // 8, h, w, 8), dtype=tdt, device=DEV)
        xd = x.to(DEV).contiguous()
        L.call("mc_pack_nchw", L.ptr(xd), n, c, c, h, w, 0, 0, None, mc, L.ptr(out), L.stream())
        return out

    def drop(self, p, st):
        return L.Dropout(L.ptr(st), LAYER, R.keep16(p))

    def gn_args(self):
        n, c, groups, h, w = self.case
        return (L.ptr(self.y), n, c, h, w, groups, L.ptr(self.stats), L.ptr(self.gamma), L.ptr(self.beta))

    def out(self):
        n, c, groups, h, w = self.case
        return Guarded((n, self.c8, h, w, 8), self.tdt)

    def forward(self, p=None, small=False):
        """(activated tensor, GroupNorm statistics the small kernel wrote or None)."""
        n, c, groups, h, w = self.case
        o, st = self.out(), state()
        dr = () if p is None else (C.byref(self.drop(p, st)),)
        sfx = "" if p is None else "_drop"
        stats = None
        if small:
            stats = Guarded((n, groups, 2), torch.float32)
            L.call("mc_gn_act_fwd_small" + sfx, L.ptr(self.y), L.ptr(self.part), self.tiles, n, c, h, w, groups, EPS,
                   L.ptr(self.gamma), L.ptr(self.beta), ACT, 1, self.mc, stats.ptr, o.ptr, None, *dr, self.st)
        else:
            L.call("mc_gn_act_fwd" + sfx, *self.gn_args(), L.POST_GN_ACT, ACT, 1, self.mc, o.ptr, None, *dr, self.st)
        torch.cuda.synchronize()
        assert o.intact() and (stats is None or stats.intact())
        assert bool((st.cpu() == state().cpu()).all()), "a kernel wrote the dropout state"
        return o.t, (None if stats is None else stats.t)

    def sources(self, kinds, factor=None):
        """mc_grad_src list of the given kinds; factor: CB8 multiplier (2 m) applied on the host to the interior."""
        n, c, groups, h, w = self.case
        out, keep = [], []
        for k in kinds:
            g, pad = {"plain": (self.grads[0], 0), "padfold": (self.grads[1], 2), "padfold1": (self.grads[2], 1)}[k]
            if factor is not None:
                g = g.clone()
                inner = g[:, :, pad:pad + h, pad:pad + w]
                inner.copy_((inner.float() * factor).to(g.dtype))
            keep.append(g)
            out.append(L.GradSrc(L.ptr(g), L.GSRC_PLAIN if k == "plain" else L.GSRC_PADFOLD, pad, 0, 1, h, w, 0, 0))
        return out, keep


@functools.lru_cache(maxsize=4)
def setup(case, prec):
    return Setup(case, prec)


# ---- forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(DT))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_half_is_twice_the_masked_activation(case, prec):
    s = setup(case, prec)
    m2 = 2.0 * mask_cb8(case, 0.5).to(DEV).float()
    for small in ([False, True] if small_ok(case) else [False]):
        a0, st0 = s.forward(None, small)
        ad, st1 = s.forward(0.5, small)
        assert not bool(torch.isnan(a0.float()).any())
        assert twice_masked(ad, a0, m2), f"small={small}"
        if small:
            assert same(st0, st1)
    c = case[1]
    if c % 8:                                                  # lanes past c_out stay exactly zero
        assert bool((ad.reshape(case[0], -1, case[3], case[4], 8)[:, -1, :, :, c % 8:] == 0).all())


@pytest.mark.parametrize("prec", list(DT))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_tenth_drops_the_restated_set(case, prec):
    s = setup(case, prec)
    n, c, groups, h, w = case
    keep = mask_cb8(case, 0.1).to(DEV)
    sc = float(R.scale(0.1))
    real = torch.zeros((1, s.c8, 1, 1, 8), dtype=torch.bool, device=DEV)
    real.view(-1)[:c] = True
    real = real.expand(n, s.c8, h, w, 8)
    for small in ([False, True] if small_ok(case) else [False]):
        a0, _ = s.forward(None, small)
        ad, _ = s.forward(0.1, small)
        assert bool((a0[real] != 0).all()), "an activation is exactly zero: the dropped set cannot be read off the output"
        assert bool(((ad == 0) == ~keep)[real].all()), f"small={small}: dropped set differs from the restatement"
        assert bool((ad[~real] == 0).all())
        want = sc * a0.double()
        err = (ad.double() - want).abs()
        tol = (2 * s.u + 2.0 ** -23) * want.abs() + (2.0 ** -24 if s.tdt == torch.float16 else 0.0)
        sel = real & keep
        worst = float((err[sel] / tol[sel].clamp_min(1e-300)).max())
        print(f"{case} {prec} small={small}: worst err / tol {worst:.3f}")
        assert bool((err[sel] <= tol[sel]).all())


# ---- backward ---------------------------------------------------------------------------------------------------------------
SOURCES = [("plain",), ("padfold",), ("padfold", "plain"), ("padfold1", "padfold")]


@pytest.mark.parametrize("kinds", SOURCES, ids=["+".join(k) for k in SOURCES])
@pytest.mark.parametrize("prec", list(DT))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_half_equals_twin_on_masked_sources(case, prec, kinds):
    s = setup(case, prec)
    n, c, groups, h, w = case
    m2 = 2.0 * mask_cb8(case, 0.5).to(DEV).float()
    gs, keep_a = s.sources(kinds)                 # the dropout entry points read g ...
    gm, keep_b = s.sources(kinds, m2)             # ... their twins 2 m g
    st = state()
    dr = C.byref(s.drop(0.5, st))

    def two(g):
        return C.byref(g[0]), (C.byref(g[1]) if len(g) > 1 else None)

    blocks = L.call("mc_gn_bwd_blocks", h, w)
    cp = s.c8 * 8
    res = {}
    for name, g, extra in (("twin", gm, ()), ("drop", gs, (dr,))):
        sfx = "_drop" if extra else ""
        part = Guarded((n, blocks, cp, 2), torch.float32)
        L.call("mc_gn_act_bwd_reduce" + sfx, *s.gn_args(), L.POST_GN_ACT, ACT, s.mc, *two(g), part.ptr, *extra, s.st)
        if name == "twin":
            m12 = torch.empty((n, groups, 2), dtype=torch.float32, device=DEV)
            L.call("mc_gn_act_bwd_finalize", part.ptr, n, blocks, c, groups, h * w, L.ptr(s.gamma), L.ptr(m12), None, None, s.st)
        dy = Guarded((n, s.c8, h, w, 8), s.gdt)
        L.call("mc_gn_act_bwd_apply" + sfx, L.ptr(s.y), n, c, h, w, groups, L.ptr(s.stats), L.ptr(m12), L.ptr(s.gamma),
               L.ptr(s.beta), L.POST_GN_ACT, ACT, s.mc, *two(g), dy.ptr, *extra, s.st)
        res[name] = [part, dy]
        if small_ok(case):
            dys, pc = Guarded((n, s.c8, h, w, 8), s.gdt), Guarded((n, cp, 2), torch.float32)
            L.call("mc_gn_act_bwd_small" + sfx, L.ptr(s.y), n, c, h, w, groups, L.ptr(s.stats), L.ptr(s.gamma), L.ptr(s.beta), ACT,
                   s.mc, *two(g), dys.ptr, pc.ptr, *extra, s.st)
            res[name] += [dys, pc]
    torch.cuda.synchronize()
    names = ["reduce partials", "dy", "dy (one launch)", "chan_sums (one launch)"]
    for k, (a, b) in enumerate(zip(res["twin"], res["drop"])):
        assert a.intact() and b.intact(), names[k]
        real = a.t if k != 0 else a.t[:, :, :c]
        got = b.t if k != 0 else b.t[:, :, :c]
        if k == 3:
            real, got = a.t[:, :c], b.t[:, :c]
        assert not bool(torch.isnan(real.float()).any()), names[k]
        assert same(got, real), f"{names[k]}: the dropout kernel differs from its twin on masked sources"
    assert bool((res["drop"][1].t.float().abs() > 0).any())
    assert bool((st.cpu() == state().cpu()).all())


# ---- the rest ---------------------------------------------------------------------------------------------------------------
def test_advance_adds_one_to_the_step_only():
    st = Guarded((4,), torch.int32, fill=None)
    st.t.copy_(state(41))
    L.call("mc_dropout_advance", st.ptr, L.stream())
    L.call("mc_dropout_advance", st.ptr, L.stream())
    torch.cuda.synchronize()
    assert st.intact()
    assert st.t.cpu().numpy().view(np.uint32).tolist() == [SEED[0], SEED[1], 43, 0]
    st.t.copy_(state(0xFFFFFFFF))
    L.call("mc_dropout_advance", st.ptr, L.stream())
    torch.cuda.synchronize()
    assert st.t.cpu().numpy().view(np.uint32).tolist() == [SEED[0], SEED[1], 0, 0]


def test_drop_forms_refuse_pooling_and_bad_descriptors():
    s = setup(CASES[1], "fp32")
    n, c, groups, h, w = s.case
    st = state()
    lib = L.load()
    o, pooled = s.out(), Guarded((n, s.c8, h // 2, w // 2, 8), s.tdt)
    stats = torch.empty((n, groups, 2), dtype=torch.float32, device=DEV)
    for pool in (2, 4):
        dr = s.drop(0.5, st)
        assert lib.mc_gn_act_fwd_drop(*s.gn_args(), L.POST_GN_ACT, ACT, pool, s.mc, o.ptr, pooled.ptr, C.byref(dr), s.st) == -2
    dr = s.drop(0.5, st)
    assert lib.mc_gn_act_fwd_small_drop(L.ptr(s.y), L.ptr(s.part), s.tiles, n, c, h, w, groups, EPS, L.ptr(s.gamma), L.ptr(s.beta),
                                        ACT, 2, s.mc, L.ptr(stats), o.ptr, pooled.ptr, C.byref(dr), s.st) == -2
    assert lib.mc_gn_act_fwd_drop(*s.gn_args(), L.POST_GN_ACT, ACT, 1, s.mc, o.ptr, None, None, s.st) == -1
    for bad in (L.Dropout(None, 0, 32768), L.Dropout(L.ptr(st), 0, 0), L.Dropout(L.ptr(st), 0, 65536)):
        assert lib.mc_gn_act_fwd_drop(*s.gn_args(), L.POST_GN_ACT, ACT, 1, s.mc, o.ptr, None, C.byref(bad), s.st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(o.t.float()).all()) and o.intact() and pooled.intact()      # nothing was launched

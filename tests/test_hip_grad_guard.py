"""Guarded optimizer step on the GPU: the ordered gradient-norm / non-finite reduction (mc_grad_guard_eval), the Adam launch
that honours its record (mc_adam_step_flat_guarded), and the Trainer's max_grad_norm / skip_nonfinite keywords around them.
Everything that can be exact is compared bit for bit: the guarded step with the guard idle against mc_adam_step_flat, the clipped
step against mc_adam_step_flat with the clipped scale, a skipped step against the state before it, captured against eager."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# one block / scalar tail only / exactly one float4 / float4 + tail / several waves / block boundary 1024 +- 1 / several
# blocks / past the grid caps of both kernels (threads loop, and a scalar tail exists)
NUMELS = [1, 3, 4, 5, 255, 1023, 1024, 1025, 10007, 2048 * 256 * 4 + 5]
ADAM = (0.9, 0.999, 1e-8, 1e-2)          # betas, eps, weight decay
LR = 2e-3


def L_():
    from pbml_mantle_convection_amd import _lib as L
    return L


def padded(x):
    """A device copy of the 1-D CPU tensor x in a buffer padded to a multiple of four floats (16-byte aligned)."""
    n = x.numel()
    t = torch.zeros((n + 3) // 4 * 4, device=DEV)
    t[:n] = x.to(DEV)
    return t


class State:
    """Parameters, Adam moments, step counter, lr, guard record and reduction workspace of one optimizer."""

    def __init__(self, n, seed=0):
        g = torch.Generator().manual_seed(1000 + seed)
        self.n = n
        self.p0 = torch.randn(n, generator=g)
        self.p = padded(self.p0)
        self.m = padded(0.1 * torch.randn(n, generator=g))
        self.v = padded(0.1 * torch.rand(n, generator=g))
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.lr = torch.full((1,), LR, device=DEV)
        self.guard = torch.zeros(L_().GRAD_GUARD_WORDS, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros(2 * L_().call("mc_grad_norm_blocks", n), dtype=torch.float64, device=DEV)

    def zero_moments(self):
        self.m.zero_()
        self.v.zero_()
        return self

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.p, self.m, self.v, self.step)]

    def record(self):
        return L_().read_grad_guard(self.guard), self.guard.cpu().numpy().tobytes()

    def evaluate(self, g, scale, max_norm, skip):
        L = L_()
        L.call("mc_grad_guard_eval", L.ptr(g), self.n, scale, max_norm, skip, L.ptr(self.ws), L.ptr(self.guard), L.ptr(self.step),
               L.stream())

    def guarded(self, g, scale, max_norm, skip):
        L = L_()
        self.evaluate(g, scale, max_norm, skip)
        L.call("mc_adam_step_flat_guarded", L.ptr(self.p), L.ptr(g), L.ptr(self.m), L.ptr(self.v), self.n, L.ptr(self.lr), *ADAM,
               scale, L.ptr(self.step), L.ptr(self.guard), L.stream())

    def plain(self, g, scale):
        L = L_()
        L.call("mc_adam_step_flat", L.ptr(self.p), L.ptr(g), L.ptr(self.m), L.ptr(self.v), self.n, L.ptr(self.lr), *ADAM, scale,
               L.ptr(self.step), L.stream())


def same(a, b, nan=False):
    """Bit-identical snapshots (NaN == NaN when `nan`)."""
    for x, y in zip(a, b):
        if nan:
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
        else:
            assert torch.equal(x, y), float((x.double() - y.double()).abs().max())


@functools.lru_cache(maxsize=None)
def grads(n, count=5):
    """`count` CPU gradients of n elements (shared by the tests of one size, never modified)."""
    g = torch.Generator().manual_seed(7 + n % 1000)
    return tuple(torch.randn(n, generator=g) for _ in range(count))


def ref_norm(g_cpu, scale):
    g64 = g_cpu.numpy().astype(np.float64)
    return scale * np.sqrt(np.sum(g64 * g64))


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", NUMELS)
def test_norm(n):
    """norm is ONE f32 rounding of the f64 value grad_scale * sqrt(sum g^2) (the accumulation is f64, so nothing else enters):
    half an ulp, <= 2^-24 relative; the bound is that, doubled."""
    gc = grads(n)[0]
    g = padded(gc)
    st = State(n)
    st.evaluate(g, 0.25, 0.0, 1)
    rec, raw = st.record()
    ref = ref_norm(gc, 0.25)
    print(f"numel {n}: norm {rec['norm']!r} ref {ref!r} rel err {abs(rec['norm'] - ref) / ref:.3e}")
    assert abs(rec["norm"] - ref) <= 2 * 2.0 ** -24 * ref
    assert (rec["nonfinite"], rec["skip"], rec["coef"], rec["skipped"], rec["consecutive"]) == (0, 0, 1.0, 0, 0)
    st.evaluate(g, 0.25, 0.0, 1)
    assert st.record()[1] == raw                      # bit-reproducible
    assert int(st.step.item()) == 2                   # the evaluation advances Adam's t


@pytest.mark.parametrize("n", NUMELS)
def test_idle_guard_is_invisible(n):
    a, b = State(n).zero_moments(), State(n).zero_moments()
    for gc in grads(n):
        g = padded(gc * 4.0)
        a.guarded(g, 0.25, 0.0, 1)
        b.plain(g, 0.25)
    same(a.snapshot(), b.snapshot())
    assert int(a.step.item()) == 5
    assert a.record()[0]["skipped"] == 0


@pytest.mark.parametrize("n", NUMELS)
def test_clipping_is_the_unguarded_step_with_the_clipped_scale(n):
    gc = grads(n)[0]
    g = padded(gc)
    ref = ref_norm(gc, 0.25)
    max_norm = float(np.float32(0.5 * ref))           # the entry point takes a float
    a, b = State(n), State(n)
    a.guarded(g, 0.25, max_norm, 1)
    rec, _ = a.record()
    want = np.float32(max_norm / (ref + 1e-6))
    print(f"numel {n}: coef {rec['coef']!r} expected {float(want)!r}")
    assert abs(np.float32(rec["coef"]) - want) <= np.spacing(want)
    assert rec["skip"] == 0 and rec["nonfinite"] == 0 and 0.0 < rec["coef"] < 1.0
    b.plain(g, float(np.float32(0.25) * np.float32(rec["coef"])))
    same(a.snapshot(), b.snapshot())


@pytest.mark.parametrize("n,offset", [(n, 0.25) for n in NUMELS] + [(n, 0.0) for n in NUMELS if n <= 10007])
def test_clipping_matches_torch(n, offset):
    """clip_grad_norm_ + torch.optim.Adam on the CPU, at test_fused_adam_matches_torch's tolerance: the kernel body is the same
    and the one new multiply is f32.

    The gradients are randn pushed away from zero by 0.25 (sign kept).  Adam's first steps move a weight by lr * g / (|g| + eps):
    a step function of g at g = 0, so an element whose decayed, clipped gradient lands within ~1e-6 of zero amplifies the last
    bit of the clip coefficient (torch sums the norm in f32) a thousandfold.  Among 2 * 10^6 plain randn elements a few land
    there, and torch's f32 result then misses this tolerance against torch's own f64 result (3 elements, 2.1e-5); with the
    offset |coef * g| >= 0.11 > weight_decay * |p| and the two f32 results agree to the rounding of p itself.  Up to 10^4
    elements none lands there with these seeds, and plain randn (offset 0) is compared as well."""
    st = State(n).zero_moments()
    ref_p = st.p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref_p], lr=LR, betas=ADAM[:2], eps=ADAM[2], weight_decay=ADAM[3])
    max_norm = 0.5 * float(np.sqrt(n))                # half of a randn gradient's expected norm: most steps clip
    clipped = 0
    for gc in grads(n):
        gc = torch.sign(gc) * (gc.abs() + offset)
        ref_p.grad = gc.clone()
        torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        opt.step()
        st.guarded(padded(gc * 4.0), 0.25, max_norm, 1)       # grad_scale 1/4 undoes the x4
        clipped += st.record()[0]["coef"] < 1.0
    assert clipped >= 1 or n == 1
    got, want = st.p[:n].double().cpu().numpy(), ref_p.detach().double().numpy()
    err = np.abs(got - want)
    print(f"numel {n} offset {offset}: max err {err.max():.3e}, clipped steps {clipped}")
    assert (err <= 1e-6 + 1e-5 * np.abs(want)).all(), err.max()
    assert int(st.step.item()) == 5


def positions(n):
    """Element 0, the last element (the scalar tail when n % 4 != 0), the last full float4, and an element of block 1."""
    pos = {0, n - 1}
    if n >= 4:
        pos.add(4 * (n // 4 - 1) + 2)
    if L_().call("mc_grad_norm_blocks", n) > 1:
        pos.add(4 * 256 + 1)                          # float4 number 256 is block 1's first
    return sorted(pos)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("n", NUMELS)
def test_nonfinite_placement(n, bad):
    clean = padded(grads(n)[0])
    cases = [[p] for p in positions(n)] + [positions(n)]
    for planted in cases:
        g = clean.clone()
        g[planted] = bad
        st = State(n)
        before = st.snapshot()
        for k in (1, 2):                              # two poisoned calls: nothing moves, the counters count
            st.guarded(g, 0.25, 0.0, 1)
            rec, _ = st.record()
            assert rec["nonfinite"] == len(planted), (planted, rec)
            assert (rec["skip"], rec["skipped"], rec["consecutive"]) == (1, k, k), (planted, rec)
            same(st.snapshot(), before)
        st.guarded(clean, 0.25, 0.0, 1)               # a clean call then trains
        rec, _ = st.record()
        after = st.snapshot()
        assert (rec["skip"], rec["consecutive"], rec["skipped"], rec["nonfinite"]) == (0, 0, 2, 0), (planted, rec)
        assert int(after[3].item()) == 1
        assert not torch.equal(after[0][:n], before[0][:n]) and bool(torch.isfinite(after[0]).all())
        # skip_nonfinite = 0: the unguarded kernel's result on the same data, NaN included
        a, b = State(n), State(n)
        a.guarded(g, 0.25, 1.0, 0)
        b.plain(g, 0.25)
        rec, _ = a.record()
        assert (rec["nonfinite"], rec["skip"], rec["coef"], rec["skipped"]) == (len(planted), 0, 1.0, 0), (planted, rec)
        same(a.snapshot(), b.snapshot(), nan=True)
        assert not bool(torch.isfinite(a.p).all())


def test_large_but_finite():
    """Four elements of 3e38: sum g^2 = 3.6e77 is an ordinary f64, the norm 6e38 rounds to +inf in f32, and the f64 coefficient
    1 / 6e38 is a subnormal f32 that scales the gradient to 0.5 per element."""
    n = 4
    g = padded(torch.full((n,), 3e38))
    st = State(n)
    st.guarded(g, 1.0, 1.0, 1)
    rec, _ = st.record()
    print(rec)
    assert rec["nonfinite"] == 0 and rec["skip"] == 0
    assert rec["norm"] == float("inf")
    assert 0.0 < rec["coef"] < 1e-37
    assert int(st.step.item()) == 1
    assert bool(torch.isfinite(st.p).all()) and not torch.equal(st.p[:n], st.p0.to(DEV))


# ---------------------------------------------------------------------------------------------------- trainer
POISON = (0, 3, 10, 10)                  # one element of gVTp


@functools.lru_cache(maxsize=None)
def batch(seed=5):
    from pbml_mantle_convection_amd.datasetio import synthetic_batch
    gVTp, uvp, scaler, paras, yc = [t.to(DEV) for t in synthetic_batch(2, 64, 122, seed, p_pred=True, device="cpu")]
    return gVTp, uvp, yc, paras, scaler              # train_step's argument order


def poisoned(seed=5):
    b = list(batch(seed))
    b[0] = b[0].clone()
    b[0][POISON] = float("nan")
    return tuple(b)


def make(prec, use_graph=False, scale_first_conv=None, **kw):
    from pbml_mantle_convection_amd.multigpu import Trainer
    from pbml_mantle_convection_amd.pytorch_networks_convae import Unet
    torch.manual_seed(3)
    m = Unet(3, 10, 16, 4, torch.device(DEV), "gelu", "reflect", "mass", use_symm=True, repeats=2, f=5, p_pred=True)
    if scale_first_conv is not None:
        with torch.no_grad():
            dict(m.named_parameters())["conv.0.layers.0.weight"].mul_(scale_first_conv)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1000], gamma=0.5)
    return Trainer(m, None, None, None, None, None, opt, sch, 0, 1, "/tmp/", p_pred=True, network="unet", loss_type="mass",
                   lambda_mom=1e-6, precision=prec, use_graph=use_graph, **kw)


def state(tr):
    torch.cuda.synchronize()
    return [tr.flat.param.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.step_count.clone()]


@functools.lru_cache(maxsize=None)
def three_steps(prec, use_graph, guarded):
    tr = make(prec, use_graph, **(dict(skip_nonfinite=True) if guarded else {}))
    assert (tr._guard is None) == (not guarded)
    for _ in range(3):
        tr.train_step(*batch())
    if guarded:
        rec = tr.grad_guard()
        assert (rec["skipped"], rec["skip"], rec["nonfinite"], rec["coef"]) == (0, 0, 0, 1.0) and rec["norm"] > 0.0
    return state(tr)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_defaults_leave_the_step_alone(prec, use_graph):
    same(three_steps(prec, use_graph, True), three_steps(prec, use_graph, False))
    same(three_steps(prec, True, True), three_steps(prec, False, True))        # captured == eager
    assert int(three_steps(prec, use_graph, True)[3].item()) == 3


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_clipping_in_the_trainer(prec):
    L = L_()
    t1 = make(prec, max_grad_norm=1e30)
    t1.train_step(*batch())
    r1 = t1.grad_guard()
    n1 = r1["norm"]
    assert r1["coef"] == 1.0 and np.isfinite(n1) and n1 > 0.0
    t2 = make(prec, max_grad_norm=0.5 * n1)
    t2.train_step(*batch())
    coef = t2.grad_guard()["coef"]
    want = np.float32(0.5 * n1 / (n1 + 1e-6))
    print(f"{prec}: norm {n1!r} coef {coef!r} expected {float(want)!r}")
    assert abs(np.float32(coef) - want) <= np.spacing(want)
    t3 = make(prec)
    t3._sync_lr()
    t3._fwd_bwd(*batch(), train=True)
    b1, b2, eps, wd = t3._adam_args()
    L.call("mc_adam_step_flat", L.ptr(t3.flat.param), L.ptr(t3.flat.grad), L.ptr(t3.exp_avg), L.ptr(t3.exp_avg_sq), t3.flat.numel,
           L.ptr(t3.lr_dev), b1, b2, eps, wd, float(np.float32(1.0) * np.float32(coef)), L.ptr(t3.step_count), L.stream())
    same(state(t2), state(t3))
    assert not torch.equal(t2.flat.param, t1.flat.param)


@functools.lru_cache(maxsize=None)
def poisoned_then_clean(prec, use_graph):
    tr = make(prec, use_graph, skip_nonfinite=True)
    before = state(tr)
    tr.train_step(*poisoned())
    same(state(tr), before)                            # parameters, both moments and step_count (0) as they were
    rec = tr.grad_guard()
    assert int(tr.step_count.item()) == 0 and rec["skipped"] == 1 and rec["skip"] == 1 and rec["nonfinite"] > 0
    tr.train_step(*batch())
    rec = tr.grad_guard()
    after = state(tr)
    assert rec["consecutive"] == 0 and rec["skipped"] == 1 and int(tr.step_count.item()) == 1
    assert bool(torch.isfinite(after[0]).all()) and not torch.equal(after[0], before[0])
    return after


@pytest.mark.parametrize("prec", ["fp32", "mixed"])
def test_poisoned_batch(prec):
    same(poisoned_then_clean(prec, True), poisoned_then_clean(prec, False))
    tr = make(prec)                                    # the contrast: what the guard is for
    tr.train_step(*poisoned())
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(tr.flat.param).all())


def test_f16_overflow_is_skipped():
    """'mixed' stores the raw convolution outputs as f16 without saturation: a first layer scaled by 1e6 overflows them."""
    tr = make("mixed", scale_first_conv=1e6, skip_nonfinite=True)
    before = state(tr)
    tr.train_step(*batch())
    rec = tr.grad_guard()
    print(rec)
    assert rec["nonfinite"] > 0 and rec["skip"] == 1
    same(state(tr), before)
    tr = make("mixed", scale_first_conv=1e6)
    tr.train_step(*batch())
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(tr.flat.param).all())


def test_consecutive_limit():
    tr = make("fp32", skip_nonfinite=True, max_skipped_in_a_row=2)
    tr.train_step(*poisoned())
    assert tr.check_guard()["consecutive"] == 1
    tr.train_step(*poisoned())
    with pytest.raises(RuntimeError, match="non-finite"):
        tr.check_guard()
    tr.train_step(*batch())
    assert tr.check_guard()["consecutive"] == 0
    assert make("fp32").check_guard() is None


def test_epoch_means_skip_the_poisoned_batch(capsys):
    def loader_item(b):
        gVTp, uvp, yc, paras, scaler = b
        return gVTp, uvp, scaler, paras, yc            # the dataset's order (Trainer._unpack)

    items = [loader_item(batch(5)), loader_item(poisoned(6)), loader_item(batch(7))]
    tr = make("fp32", skip_nonfinite=True)
    tr.train_data, tr.cv_data = items, []
    tr._run_epoch(0)
    out = capsys.readouterr().out
    assert out.count("[mantle]") == 1 and "1 of 3 optimizer steps skipped" in out
    ref = make("fp32", skip_nonfinite=True)
    outs = [ref._run_batch(x, y, sc, True, paras=pa, yc=yc, sync=False).double().clone() for x, y, sc, pa, yc in items]
    assert not bool(torch.isfinite(outs[1]).all())
    want = ((outs[0] + outs[2]) / 2)[:6].tolist()
    print(tr.losses, want)
    assert np.isfinite(tr.losses).all()
    assert tr.losses == pytest.approx(want, rel=1e-12, abs=0.0)
    assert tr.grad_guard()["skipped"] == 1

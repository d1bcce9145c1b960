"""GPU, kernel level through the C ABI: the series-scoring gather, row pass and finalize (mc_series_*) -- the gather against
mc_ts_build_input on the gathered arrays (bit equality), table and profile against the numpy restatement of the contract
(series_score_ref), a snapshot alone against the same snapshot inside a batch, and a list walked by a batch that does not divide
its length.  Outputs are NaN-prefilled and sit between sentinel bands."""
import functools

import numpy as np
import pytest
import torch

import eval_seams as S
import series_score_ref as R
from test_hip_rollout import DEV, Guarded, dev, grid

pytestmark = pytest.mark.gpu

SIZES = [(3, 3, 3), (5, 7, 70), (4, 33, 130)]      # a 1 x 1 interior; a ragged row longer than a wave; several rows a block, 3 waves a row
# tests/eval_seams.py: heights at which k_series_finalize takes exactly one pass, a second pass of one row, three passes; a
# field whose gather takes the grid-stride pass
FINALIZE_SIZES = SIZES + S.SERIES_SHAPES
F64, I32, F32 = torch.float64, torch.int32, torch.float32
INV = S.INV                                       # two simulations, different velocity scales


@functools.lru_cache(maxsize=None)
def case(N, H, W):
    """A store of N snapshots of two simulations (the second half belongs to simulation 1) and one prediction per snapshot in
    the scaled space: the scaled truth (0.1 to 0.8 in size) plus a smooth error of about 0.1."""
    f = S.series_fields(N, H, W)
    u, v, T, sim, prev, pred = f["u"], f["v"], f["T"], f["sim"], f["prev"], f["pred"]
    paras = np.array([[1.5, 1e6, 10.0], [4.0, 1e8, 60.0]])
    nd = np.array([[0.15, 0.0, 0.5], [0.4, 0.51, 0.89]])
    xc, yc = grid(H, W)
    host = dict(u=u.astype(np.float32), v=v.astype(np.float32), sim=sim, prev=prev, pred=pred)
    return dict(N=N, H=H, W=W, host=host, u=dev(u), v=dev(v), T=dev(T), sim=dev(sim, I32), prev=dev(prev, I32), paras=dev(paras),
                nd=dev(nd), inv=dev(INV), xc=dev(xc), yc=dev(yc), ycc=dev(0.9 * yc), pred=dev(pred))


def run(c, idx, b, steps=None, start=0, prev=None, inv=None, uv=None, stride=None):
    """set_cursor(start), then `steps` times { row pass, finalize } with b slots (default: as many as walk the list).  The
    prediction of item j is pred[idx[j]].  Returns table, profile, the cursor and whether every guard band is intact."""
    from pbml_mantle_convection_amd import _lib as L
    N, H, W = c["N"], c["H"], c["W"]
    idx = np.asarray(idx, dtype=np.int32)
    n = idx.shape[0]
    steps = -(-(n - start) // b) if steps is None else steps
    out = c["pred"][torch.from_numpy(idx.astype(np.int64)).to(DEV)].contiguous()
    g = dict(table=Guarded((n, 10), F64, float("nan")), profile=Guarded((n, 2, H), F64, float("nan")),
             rows=Guarded((b, 10, H), F64, float("nan")), cursor=Guarded((1,), I32, -1))
    idx_d = dev(idx, I32)
    u, v = uv if uv is not None else (c["u"], c["v"])
    s = L.stream()
    L.call("mc_series_set_cursor", g["cursor"].ptr, start, n, s)
    for k in range(steps):
        at = min(start + k * b, n - 1)                       # (a step past the end of the list reads no prediction at all)
        base = out.data_ptr() + at * 3 * H * W * 4
        L.call("mc_series_score", base, base + H * W * 4, 3 * H * W, L.ptr(u), L.ptr(v), stride or H * W, L.ptr(c["sim"]),
               L.ptr(c["prev"] if prev is None else prev), L.ptr(c["inv"] if inv is None else inv), L.ptr(idx_d), g["cursor"].ptr, n, N, 2,
               b, H, W, g["rows"].ptr, s)
        L.call("mc_series_score_finalize", g["rows"].ptr, L.ptr(idx_d), g["cursor"].ptr, n, N, b, H, W, g["table"].ptr,
               g["profile"].ptr, s)
    torch.cuda.synchronize()
    return dict(table=g["table"].t.cpu(), profile=g["profile"].t.cpu(), cursor=int(g["cursor"].t.cpu()[0]),
                intact=all(x.intact() for x in g.values()))


@functools.lru_cache(maxsize=None)
def whole(N, H, W):
    """Every snapshot in store order, one step of N slots.  Computed once, shared, never modified."""
    return run(case(N, H, W), list(range(N)), N)


@functools.lru_cache(maxsize=None)
def reference(N, H, W):
    h = case(N, H, W)["host"]
    return R.score(h["pred"][:, 0], h["pred"][:, 1], h["u"], h["v"], h["sim"], h["prev"], INV, list(range(N)))


def same(a, b):
    """Bit equality, NaN == NaN."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def gather(c, idx, b, cursor, T=None, stride=None):
    from pbml_mantle_convection_amd import _lib as L
    N, H, W = c["N"], c["H"], c["W"]
    idx = np.asarray(idx, dtype=np.int32)
    n = idx.shape[0]
    out, cur = Guarded((b, 7, H, W), F32, float("nan")), Guarded((1,), I32, -1)
    idx_d = dev(idx, I32)
    s = L.stream()
    L.call("mc_series_set_cursor", cur.ptr, cursor, n, s)
    L.call("mc_series_build_input", L.ptr(c["T"] if T is None else T), stride or H * W, L.ptr(c["sim"]), L.ptr(c["xc"]), L.ptr(c["yc"]),
           L.ptr(c["ycc"]), L.ptr(c["paras"]), L.ptr(c["nd"]), L.ptr(idx_d), cur.ptr, n, N, 2, b, H, W, out.ptr, s)
    snaps = torch.from_numpy(idx[[min(cursor + k, n - 1) for k in range(b)]].astype(np.int64)).to(DEV)
    sims = c["sim"][snaps].long()
    Tg, pg, ng = c["T"][snaps].contiguous(), c["paras"][sims].contiguous(), c["nd"][sims].contiguous()
    want = Guarded((b, 7, H, W), F32, float("nan"))
    L.call("mc_ts_build_input", L.ptr(Tg), L.ptr(c["xc"]), L.ptr(c["yc"]), L.ptr(c["ycc"]), L.ptr(pg), L.ptr(ng), b, H, W, want.ptr, s)
    torch.cuda.synchronize()
    assert out.intact() and want.intact() and cur.intact() and int(cur.t[0]) == cursor       # the gather leaves the cursor alone
    return out.t.cpu(), want.t.cpu()


@pytest.mark.parametrize("N,H,W", SIZES + [S.GATHER_SHAPE])
def test_gather_equals_ts_build_input(N, H, W):
    c = case(N, H, W)
    idx = [(3 * j + 1) % N for j in range(N + 2)]            # permuted, with repeats
    for b, cursor in ((N + 2, 0), (3, 0), (3, N)):           # the whole list; its head; a tail of 2 items in 3 slots
        got, want = gather(c, idx, b, cursor)
        assert bool(torch.isfinite(want).all()) and torch.equal(got, want), (b, cursor)
    if N == 1:                                               # (one snapshot: the grid-stride pass is what this size is here for)
        assert (N, H, W) == S.GATHER_SHAPE and bool((got[:, 6] == c["T"][0].cpu()).all())
        return
    got, _ = gather(c, [0, N - 1], 2, 0)                     # snapshots and simulations differ, so a mixed-up slot would show
    assert not torch.equal(got[0, 6], got[1, 6]) and not torch.equal(got[0, 3:6], got[1, 3:6]) and not torch.equal(got[0, 2], got[1, 2])


@pytest.mark.parametrize("N,H,W", FINALIZE_SIZES)
def test_table_and_profile_against_numpy(N, H, W):
    got = whole(N, H, W)
    table, profile, gate, pgate = reference(N, H, W)
    t, p = got["table"].numpy(), got["profile"].numpy()
    assert got["intact"] and got["cursor"] == N
    for j in range(N):
        for q in range(10):
            print(f"item {j} {R.NAMES[q]}: got {t[j, q]!r} want {table[j, q]!r} |diff| {abs(t[j, q] - table[j, q]):.3e} gate {gate[j, q]:.3e}")
    print(f"worst |got - want| / gate: table {S.worst_ratio(t, table, gate):.3e} profiles {S.worst_ratio(p, profile, pgate):.3e}")
    assert np.array_equal(t[:, R.MAX_COLS], table[:, R.MAX_COLS])                                 # maxima are exact
    assert R.close(t, table, gate) and R.close(p, profile, pgate)
    assert np.isfinite(t[:, [0, 1, 4, 5, 6, 7, 8, 9]]).all() and (t[:, [0, 1, 4, 5, 6, 7]] > 0).all()
    if H > 3:
        assert (t[:, 8:] > 0).all()
    # cross-check: the mean of the error profile over the rows is the MAE
    assert np.allclose(p.mean(-1), t[:, :2], rtol=1e-13, atol=0)


@pytest.mark.parametrize("N,H,W", SIZES)
def test_first_snapshots_have_no_baseline(N, H, W):
    c, t = case(N, H, W), whole(N, H, W)["table"].numpy()
    first = c["host"]["prev"] < 0
    assert first.sum() == 2 and np.isnan(t[first][:, 2:4]).all() and np.isfinite(t[~first][:, 2:4]).all() and (t[~first][:, 2:4] > 0).all()
    # a store whose snapshots all lack a predecessor: both columns NaN everywhere, nothing else moves
    none = run(c, list(range(N)), N, prev=dev(np.full(N, -1), I32))
    assert none["intact"] and bool(torch.isnan(none["table"][:, 2:4]).all())
    keep = [0, 1, 4, 5, 6, 7, 8, 9]
    assert same(none["table"][:, keep].contiguous(), whole(N, H, W)["table"][:, keep].contiguous()) and same(none["profile"], whole(N, H, W)["profile"])


@pytest.mark.parametrize("N,H,W", FINALIZE_SIZES)
def test_alone_equals_inside_a_batch(N, H, W):
    c, ref = case(N, H, W), whole(N, H, W)
    for s in range(N):
        one = run(c, [s], 1)
        assert one["intact"] and one["cursor"] == 1
        assert same(one["table"][0], ref["table"][s]) and same(one["profile"][0], ref["profile"][s]), s
    wide = run(c, [N - 1], 4)                                # one item in four slots
    assert wide["intact"] and wide["cursor"] == 1 and same(wide["table"][0], ref["table"][N - 1])


def test_list_walked_by_a_batch_that_does_not_divide_it():
    N, H, W = SIZES[1]
    c, ref = case(N, H, W), whole(N, H, W)
    assert N == 5
    two = run(c, list(range(5)), 2, steps=2)                 # after two steps: four rows written, the fifth still NaN
    assert two["cursor"] == 4 and bool(torch.isnan(two["table"][4]).all()) and bool(torch.isnan(two["profile"][4]).all())
    assert same(two["table"][:4], ref["table"][:4])
    three = run(c, list(range(5)), 2)                        # three steps fill all five rows; the sixth slot writes nothing:
    assert three["intact"] and three["cursor"] == 5          # ... the bands behind row 4 are intact, the cursor stops at 5
    assert same(three["table"], ref["table"]) and same(three["profile"], ref["profile"])
    four = run(c, list(range(5)), 2, steps=4)                # a step past the end of the list writes nothing at all
    assert four["intact"] and four["cursor"] == 5 and same(four["table"], ref["table"])
    late = run(c, list(range(5)), 2, start=3)                # a cursor set into the list: rows before it stay NaN
    assert late["cursor"] == 5 and bool(torch.isnan(late["table"][:3]).all()) and same(late["table"][3:], ref["table"][3:])


@pytest.mark.parametrize("N,H,W", FINALIZE_SIZES)
def test_permuted_and_repeated_list(N, H, W):
    c, ref = case(N, H, W), whole(N, H, W)
    idx = [(3 * j + 1) % N for j in range(N + 2)]
    got = run(c, idx, 2)
    assert got["intact"] and got["cursor"] == N + 2
    sel = torch.tensor(idx)
    assert same(got["table"], ref["table"][sel]) and same(got["profile"], ref["profile"][sel])
    if len(set(idx)) < N:                                    # (N a multiple of 3: that list names one snapshot)
        idx = [(2 * j + 1) % N for j in range(N + 2)]
        got = run(c, idx, 2)
        sel = torch.tensor(idx)
        assert len(set(idx)) == N and got["intact"] and got["cursor"] == N + 2
        assert same(got["table"], ref["table"][sel]) and same(got["profile"], ref["profile"][sel])


def test_simulations_use_their_own_scale():
    N, H, W = SIZES[2]
    c, ref = case(N, H, W), whole(N, H, W)
    sim = c["host"]["sim"]
    swapped = run(c, list(range(N)), N, inv=dev(INV[::-1].copy()))
    t, s = ref["table"].numpy(), swapped["table"].numpy()
    ratio = float(INV[1]) / float(INV[0])
    for j in range(N):
        r = ratio if sim[j] == 0 else 1.0 / ratio
        # max|ut| scales with it up to one f32 rounding on either side; a residual is built from four products, each half an
        # ulp of at most max|ut| or max|vt| off, with weights 0.5: 2^-24 max on either side (bounds: twice that)
        assert abs(s[j, 4] - r * t[j, 4]) <= 2.0 ** -22 * r * t[j, 4], j
        assert abs(s[j, 9] - r * t[j, 9]) <= 2.0 ** -22 * r * max(t[j, 4], t[j, 5]) and s[j, 9] > 0, j
    assert t[0, 4] == float(np.abs(c["host"]["u"][0] * INV[0]).max()) and t[N - 1, 5] == float(np.abs(c["host"]["v"][N - 1] * INV[1]).max())


def test_store_read_in_place_through_its_stride():
    """T, u, v as channel 0 of [N,2,H,W] tensors (snapshot stride 2 H W, channel 1 NaN): the same bits as the dense store.  At
    5 x 7 x 70 and where the finalize takes three passes."""
    for N, H, W in (SIZES[1], S.SERIES_SHAPES[2]):
        c, ref = case(N, H, W), whole(N, H, W)
        wide = lambda a: torch.stack([a, torch.full_like(a, float("nan"))], 1).contiguous()  # noqa: E731
        got = run(c, list(range(N)), 3, uv=(wide(c["u"]), wide(c["v"])), stride=2 * H * W)
        assert got["intact"] and same(got["table"], ref["table"]) and same(got["profile"], ref["profile"])
        a, want = gather(c, [N - 1, 0, 2], 3, 0, T=wide(c["T"]), stride=2 * H * W)
        assert torch.equal(a, want)

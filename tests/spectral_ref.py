"""f64 restatement of the spectral layer (SpectralConv2d / SpectralFluidLayer) and of its two linear maps, written from
the formulas, with no FFT: the layer keeps the modes K1 = (0, 1, 2, 3, H-4, H-3, H-2, H-1) x K2 = (0, 1, 2, 3) of rfft2, so

    analysis   A(t)[n,c,k1,k2] = sum_{h,w} t[n,c,h,w] e^{-i theta}        theta = 2 pi (k1 h / H + k2 w / W)
    synthesis  S(C)[n,c,h,w]   = sum_{k1,k2} Re(C[n,c,k1,k2] e^{+i theta})
    forward    y = S(gamma * sum_i A(x)[n,i] Wt[i,o])                      gamma[k2] = (1, 2, 2, 2) / (H W)
    backward   G = gamma A(dy);  dWt[i,o] = sum_n conj(A(x)[n,i]) G[n,o];  dx = S(sum_o conj(Wt[i,o]) G[n,o])

with Wt = cat(weights1, weights2, dim=2).  tests/test_spectral_host.py pins it to the reference's own layer
(tests/golden/g24_spectral_layer.npz); the GPU tests compare the kernels with it.  Also the case tables of the kernel
tests and the perturbed variants that show their comparison can see a wrong kernel."""
import numpy as np
import torch

U32 = 2.0 ** -24                                # unit roundoff of f32
ROUNDINGS = 161                                 # the kernels' rounding cap (160, csrc/spectral.hip) plus one
STORE_U = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
STORE_F = {"f32": 0.0, "bf16": 0.0, "f16": 2.0 ** -24}       # f16 subnormal spacing

# kernel-test cases (H, W, c), all with N = 2: the minimum (the two K1 blocks adjacent, less than one channel block); odd
# in both directions with two ragged channel blocks; the deployed trunk's coarsest level; a plain one; two 32-row chunks x
# two 256-column strips with ragged remainders in both
CASES = [(8, 8, 3), (9, 11, 11), (8, 31, 8), (16, 63, 16), (37, 300, 24)]
CASE_N = 2
MIX_CASES = [(3, 5), (11, 16), (16, 16)]        # c_i -> c_o, N = 3 (the ordered dW sum)
MIX_N = 3


def k1_list(H):
    return [0, 1, 2, 3, H - 4, H - 3, H - 2, H - 1]


def tables64(H, W):
    """The engine's twiddle tables in exact f64: rowtw [H][5][2], coltw [W][4][2] = (cos, sin)(2 pi (k j mod n) / n)."""
    def tab(n, ks):
        r = (np.arange(n, dtype=np.int64)[:, None] * np.arange(ks, dtype=np.int64)[None, :]) % n
        a = 2.0 * np.pi * r.astype(np.float64) / n
        return np.stack([np.cos(a), np.sin(a)], -1)
    return tab(H, 5), tab(W, 4)


def phases_from_tables(rowtw, coltw):
    """(E1 [8][H], E2 [4][W]) = e^{-2 pi i k1 h / H}, e^{-2 pi i k2 w / W} from tables in the engine's layout (any float type,
    promoted to f64): +k rows are (cos, -sin), the rows of the second block -4..-1 are (cos, +sin) of |k|."""
    r = np.asarray(rowtw, np.float64)
    c = np.asarray(coltw, np.float64)
    E1 = np.stack([r[:, k, 0] - 1j * r[:, k, 1] for k in (0, 1, 2, 3)] + [r[:, k, 0] + 1j * r[:, k, 1] for k in (4, 3, 2, 1)], 0)
    E2 = (c[:, :, 0] - 1j * c[:, :, 1]).T
    return E1, np.ascontiguousarray(E2)


def phases_exact(H, W, k1=None, row_shift=0, sign=-1.0):
    """The same phases computed directly; the keywords build the perturbed variants (another K1 list, the row table shifted by
    row_shift rows, e^{+i theta})."""
    k1 = np.asarray(k1_list(H) if k1 is None else k1, np.int64)
    h = (np.arange(H, dtype=np.int64) + row_shift) % H
    E1 = np.exp(sign * 2j * np.pi * ((k1[:, None] * h[None, :]) % H) / H)
    E2 = np.exp(sign * 2j * np.pi * ((np.arange(4, dtype=np.int64)[:, None] * np.arange(W, dtype=np.int64)[None, :]) % W) / W)
    return E1, E2


def _abs_parts(E1, E2):
    """|Re|, |Im| bounds of the product E1[k,h] E2[q,w] term by term."""
    a1, b1, a2, b2 = np.abs(E1.real), np.abs(E1.imag), np.abs(E2.real), np.abs(E2.imag)
    return (a1, b1, a2, b2)


def analysis(t, E1, E2):
    """A(t) [N, C, 8, 4] complex128."""
    return np.einsum("nchw,kh,qw->nckq", np.asarray(t, np.float64), E1, E2, optimize=True)


def analysis_abs(t, E1, E2):
    """The same expression on absolute values, separately for the real and the imaginary part: [N, C, 8, 4, 2]."""
    a1, b1, a2, b2 = _abs_parts(E1, E2)
    t = np.abs(np.asarray(t, np.float64))
    re = np.einsum("nchw,kh,qw->nckq", t, a1, a2, optimize=True) + np.einsum("nchw,kh,qw->nckq", t, b1, b2, optimize=True)
    im = np.einsum("nchw,kh,qw->nckq", t, a1, b2, optimize=True) + np.einsum("nchw,kh,qw->nckq", t, b1, a2, optimize=True)
    return np.stack([re, im], -1)


def synthesis(C, E1, E2):
    """S(C) [N, C, H, W] f64 (E1, E2 are the analysis phases; the synthesis uses their conjugates)."""
    return np.einsum("nckq,kh,qw->nchw", C, E1.conj(), E2.conj(), optimize=True).real


def synthesis_abs(C, E1, E2):
    a1, b1, a2, b2 = _abs_parts(E1, E2)
    cr, ci = np.abs(C.real), np.abs(C.imag)
    zr = lambda c: np.einsum("nckq,kh,qw->nchw", c, a1, a2, optimize=True) + np.einsum("nckq,kh,qw->nchw", c, b1, b2, optimize=True)  # noqa: E731
    zi = lambda c: np.einsum("nckq,kh,qw->nchw", c, a1, b2, optimize=True) + np.einsum("nckq,kh,qw->nchw", c, b1, a2, optimize=True)  # noqa: E731
    return zr(cr) + zi(ci)


def gamma(H, W, factor2=True):
    return np.array([1.0, 2.0, 2.0, 2.0] if factor2 else [1.0, 1.0, 1.0, 1.0]) / float(H * W)


def wt(w1, w2):
    """[c_i, c_o, 8, 4] complex128 from the two parameters [c_i, c_o, 4, 4]."""
    return np.concatenate([np.asarray(w1, np.complex128), np.asarray(w2, np.complex128)], 2)


def mix_fwd(xhat, Wt, gam):
    return np.einsum("nikq,iokq->nokq", xhat, Wt, optimize=True) * gam


def mix_fwd_abs(xhat, Wt, gam):
    """[N, c_o, 8, 4, 2]: the real and imaginary parts' expressions on absolute values."""
    xr, xi, wr, wi = np.abs(xhat.real), np.abs(xhat.imag), np.abs(Wt.real), np.abs(Wt.imag)
    e = lambda a, b: np.einsum("nikq,iokq->nokq", a, b, optimize=True)  # noqa: E731
    return np.stack([(e(xr, wr) + e(xi, wi)) * gam, (e(xr, wi) + e(xi, wr)) * gam], -1)


def mix_bwd(xhat, Wt, G):
    """(dWt [c_i, c_o, 8, 4], dx coefficients [N, c_i, 8, 4]) from G = gamma A(dy)."""
    return (np.einsum("nikq,nokq->iokq", xhat.conj(), G, optimize=True), np.einsum("iokq,nokq->nikq", Wt.conj(), G, optimize=True))


def mix_bwd_abs(xhat, Wt, G):
    xr, xi, wr, wi, gr, gi = (np.abs(v) for v in (xhat.real, xhat.imag, Wt.real, Wt.imag, G.real, G.imag))
    ew = lambda a, b: np.einsum("nikq,nokq->iokq", a, b, optimize=True)  # noqa: E731
    ex = lambda a, b: np.einsum("iokq,nokq->nikq", a, b, optimize=True)  # noqa: E731
    return (np.stack([ew(xr, gr) + ew(xi, gi), ew(xr, gi) + ew(xi, gr)], -1),
            np.stack([ex(wr, gr) + ex(wi, gi), ex(wr, gi) + ex(wi, gr)], -1))


def conv_fwd(x, w1, w2):
    """SpectralConv2d.forward in f64."""
    H, W = x.shape[-2:]
    E1, E2 = phases_exact(H, W)
    return synthesis(mix_fwd(analysis(x, E1, E2), wt(w1, w2), gamma(H, W)), E1, E2)


def conv_bwd(x, w1, w2, dy):
    """(dx, dweights1, dweights2); a complex gradient is d/dRe + i d/dIm, what torch keeps in .grad."""
    H, W = x.shape[-2:]
    E1, E2 = phases_exact(H, W)
    dWt, dxc = mix_bwd(analysis(x, E1, E2), wt(w1, w2), analysis(dy, E1, E2) * gamma(H, W))
    return synthesis(dxc, E1, E2), dWt[:, :, :4], dWt[:, :, 4:]


_ACTS = {"gelu": torch.nn.functional.gelu, "tanh": torch.tanh, "relu": torch.relu, "silu": torch.nn.functional.silu,
         "selu": torch.selu, "elu": torch.nn.functional.elu}


def layer_torch(x, w1, w2, gn_w, gn_b, act):
    """SpectralFluidLayer.forward on f64 / complex128 torch tensors (differentiable): the truncated DFT as dense phase
    matrices, GroupNorm with int(c_o / 4) groups, activation."""
    H, W = x.shape[-2:]
    E1, E2 = (torch.from_numpy(e) for e in phases_exact(H, W))
    xhat = torch.einsum("nchw,kh,qw->nckq", x.to(torch.complex128), E1, E2)
    co = torch.einsum("nikq,iokq->nokq", xhat, torch.cat([w1, w2], 2)) * torch.from_numpy(gamma(H, W))
    y = torch.einsum("nckq,kh,qw->nchw", co, E1.conj(), E2.conj()).real
    c_o = y.shape[1]
    return _ACTS[act](torch.nn.functional.group_norm(y, int(c_o / 4), gn_w, gn_b, 1e-5))


def bound(ref, s_abs, store="f32"):
    """The kernel tests' bound per element, E + u (|ref| + E) + f with E = 161 * 2^-24 * S: S the reference's expression on
    absolute values, u / f the relative / absolute rounding of the store type."""
    E = ROUNDINGS * U32 * s_abs
    return E + STORE_U[store] * (np.abs(ref) + E) + STORE_F[store]


def draw(shape, seed, store="f32", scale=1.0):
    """Standard normal draws rounded to the element type, as f64."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g, dtype=torch.float32) * scale
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[store]
    return t.to(dt).to(torch.float64).numpy()


def draw_complex(shape, seed, scale=1.0):
    v = draw(tuple(shape) + (2,), seed, scale=scale)
    return v[..., 0] + 1j * v[..., 1]

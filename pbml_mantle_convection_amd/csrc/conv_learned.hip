// Learned padding (BoundaryLearnedConvolution2D, reference pytorch_networks_convae.py:802-1065): the FRAME of the output --
// every pixel that one of the eight border banks produces -- in one launch per direction.  The main bank stays on the
// library's conv kernels (mc_conv2d / mc_conv2d_wgrad); these kernels read X / dY in place, so no strip is ever cut out.
//
// Work decomposition (forward and input gradient): one wave owns 16 pixels x 16 output channels.  Lane (p = lane & 15,
// q = lane >> 4) ends with the four channels 16 tile + 4 q .. + 3 of pixel p -- half a CB8 vector, one 8 / 16 byte store.
//   16-bit types: v_mfma_f32_16x16x32_{bf16,f16} with A = filter fragment (M = 16 output channels) and B = the pixels'
//     CB8 vectors (N = 16 pixels); one K-step = four (channel block, tap) pairs x 8 channels, so every operand is ONE
//     16-byte load (B straight from the activation tensor, A from the bank, 1 KB contiguous per wave and step).
//   f32 (the parity mode): the same tiles and bank layout on plain FMAs.
// bank (forward):        [bank 8][co tile][pair j = cb * k*k + tap, padded to 16][co 16][ci 8]
// bank (input gradient): [bank 8][ci tile][pair j = cbo * k*k + tap, padded to 16][ci 16][co 8]    (same taps: the gather
//   below is written over input pixels, so no rotated bank is needed)
// The filter gradient reduces over pixels: per-slice partial slabs in a fixed decomposition (16-bit: MFMA with M = output
// channels, N = input channels, K = 32 pixels, operands gathered; f32: FMAs), then one reduce launch that folds the mirrored
// filters and accumulates -- no atomics, no dependence on block order.
#include "conv_common.h"
#include <type_traits>

using lbf16x8 = __attribute__((ext_vector_type(8))) short;
using lf16x8 = __attribute__((ext_vector_type(8))) _Float16;
using lf32x4 = __attribute__((ext_vector_type(4))) float;

namespace {

struct LReg { int sy, sx, sh, sw, dy, dx, rh, rw; };   // input rectangle, output origin, output rectangle of one bank

struct LGeom {
  int N, H, W, Ho, Wo, K, KK, Cin, Cout, CBin, CBout;
  int CT, IT;            // 16-channel tiles of the output / input channels
  int J, Jp, Jd, Jdp;    // (channel block, tap) pairs of the forward / input-gradient reduction, padded to 16
  int U, nh;             // unique filters, x-mirrored pairs
  int pad_x, pad_y, fx, fy, mh, mw;
  int nrb, ncb;          // rows / columns of the border bands (min(h, 2 pad_y), min(w, 2 pad_x))
  int band_pix;          // input pixels in the bands
  int frame_groups;      // 16-pixel groups of the eight output rectangles, per sample
  int dtype;
};

// bank index: bottom_left, bottom, bottom_right, left, right, top_left, top, top_right (row class x column class without
// (middle, middle)).  "bottom" is cut from the LAST input rows and lands in the FIRST output rows (reference :1057-1060).
__host__ __device__ __forceinline__ LReg l_region(const LGeom& g, int b) {
  const int id = b < 4 ? b : b + 1, rc = id / 3, cc = id - 3 * rc;
  LReg R;
  R.sy = rc == 0 ? g.H - g.pad_y : 0;
  R.sh = rc == 1 ? g.H : g.pad_y;
  R.dy = rc == 0 ? 0 : (rc == 1 ? g.fy : g.fy + g.mh);
  R.sx = cc == 2 ? g.W - g.pad_x : 0;
  R.sw = cc == 1 ? g.W : g.pad_x;
  R.dx = cc == 0 ? 0 : (cc == 1 ? g.fx : g.fx + g.mw);
  R.rh = R.sh - g.K + 1;
  R.rw = R.sw - g.K + 1;
  return R;
}

int l_geom(const mc_learned_desc* d, LGeom& g) {
  if (!d) return MC_EINVAL;
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c_in <= 0 || d->c_out <= 0 || d->bc_x < 1 || d->bc_y < 1) return MC_EINVAL;
  if (d->k != 3 && d->k != 5) return MC_EUNSUPPORTED;
  if (d->dtype != MC_F32 && d->dtype != MC_BF16 && d->dtype != MC_MIX16) return MC_EUNSUPPORTED;
  if (d->sym_h < 0 || (d->sym_h & 1) || d->sym_h > d->c_out) return MC_EUNSUPPORTED;
  if (d->bc_x > (1 << 20) || d->bc_y > (1 << 20)) return MC_EUNSUPPORTED;
  g.K = d->k; g.KK = d->k * d->k;
  g.pad_x = (d->k == 5 ? d->k + 1 : d->k) + (d->bc_x - 1);
  g.pad_y = (d->k == 5 ? d->k + 1 : d->k) + (d->bc_y - 1);
  if (d->h < d->k || d->w < d->k || d->h < g.pad_y || d->w < g.pad_x) return MC_EUNSUPPORTED;
  if ((long)d->h * d->w > (1L << 28) || (long)d->n * d->h * d->w > (1L << 30)) return MC_EUNSUPPORTED;
  g.N = d->n; g.H = d->h; g.W = d->w; g.Cin = d->c_in; g.Cout = d->c_out;
  g.fx = g.pad_x - g.K + 1; g.fy = g.pad_y - g.K + 1; g.mh = g.H - g.K + 1; g.mw = g.W - g.K + 1;
  g.Ho = g.mh + 2 * g.fy; g.Wo = g.mw + 2 * g.fx;
  g.CBin = (g.Cin + 7) / 8; g.CBout = (g.Cout + 7) / 8; g.CT = (g.Cout + 15) / 16; g.IT = (g.Cin + 15) / 16;
  g.J = g.CBin * g.KK; g.Jp = (g.J + 15) & ~15; g.Jd = g.CBout * g.KK; g.Jdp = (g.Jd + 15) & ~15;
  g.nh = d->sym_h / 2; g.U = g.Cout - g.nh;
  g.nrb = g.H < 2 * g.pad_y ? g.H : 2 * g.pad_y;
  g.ncb = g.W < 2 * g.pad_x ? g.W : 2 * g.pad_x;
  g.band_pix = g.nrb * g.W + (g.H - g.nrb) * g.ncb;
  g.frame_groups = 0;
  for (int b = 0; b < 8; ++b) { const LReg R = l_region(g, b); g.frame_groups += (R.rh * R.rw + 15) / 16; }
  g.dtype = d->dtype;
  return MC_OK;
}

size_t l_bank_elems(const LGeom& g, int dgrad) {
  return dgrad ? (size_t)8 * g.IT * g.Jdp * 128 : (size_t)8 * g.CT * g.Jp * 128;
}

// filter-gradient decomposition: every bank's (sample, pixel) visits are cut into slices of SL; one partial slab per slice
//   slab: [tap][co tile][ci tile][co 16][ci 16] f32, then the bias sums [co tile][16]
size_t l_slab_floats(const LGeom& g) { return (size_t)g.KK * g.CT * g.IT * 256 + (size_t)g.CT * 16; }
void l_wgrad_plan(const LGeom& g, int& SL, int& S) {
  const size_t slab = l_slab_floats(g) * sizeof(float);
  long smax = (long)((64ul << 20) / slab);
  smax = smax < 8 ? 8 : (smax > 1024 ? 1024 : smax);
  long V = 0;
  for (int b = 0; b < 8; ++b) { const LReg R = l_region(g, b); V += (long)g.N * R.rh * R.rw; }
  long sl = (V + smax - 1) / smax;
  const long slmin = g.dtype == MC_F32 ? 64 : 32 * 4;          // (16-bit: one 32-visit MFMA chunk per wave)
  SL = (int)(sl < slmin ? slmin : sl);
  S = 0;
  for (int b = 0; b < 8; ++b) { const LReg R = l_region(g, b); S += (int)(((long)g.N * R.rh * R.rw + SL - 1) / SL); }
}

// ---- element access ----------------------------------------------------------------------------
template <typename T> struct L4;
template <> struct L4<float> {
  static __device__ __forceinline__ void ld(const float* p, float (&o)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  }
  static __device__ __forceinline__ void st(float* p, const float (&o)[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }
  static __device__ __forceinline__ float ld1(const float* p) { return *p; }
};
template <> struct L4<bf16_t> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float (&o)[4]) {
    const uint2 a = *reinterpret_cast<const uint2*>(p);
    o[0] = __uint_as_float(a.x << 16); o[1] = __uint_as_float(a.x & 0xffff0000u);
    o[2] = __uint_as_float(a.y << 16); o[3] = __uint_as_float(a.y & 0xffff0000u);
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float (&o)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pk_bf16(o[0], o[1]), pk_bf16(o[2], o[3]));
  }
  static __device__ __forceinline__ float ld1(const bf16_t* p) { return bf2f(*p); }
};
template <> struct L4<f16_t> {
  static __device__ __forceinline__ void ld(const f16_t* p, float (&o)[4]) {
    const uint2 a = *reinterpret_cast<const uint2*>(p);
    const mc_f32x2 x = unpk_f16(a.x), y = unpk_f16(a.y);
    o[0] = x.x; o[1] = x.y; o[2] = y.x; o[3] = y.y;
  }
  static __device__ __forceinline__ void st(f16_t* p, const float (&o)[4]) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pk_f16(o[0], o[1]), pk_f16(o[2], o[3]));
  }
  static __device__ __forceinline__ float ld1(const f16_t* p) { return (float)__builtin_bit_cast(_Float16, p->v); }
};

template <bool H16> __device__ __forceinline__ lf32x4 l_mfma(uint4 a, uint4 b, lf32x4 c) {
  if constexpr (H16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lf16x8, a), __builtin_bit_cast(lf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lbf16x8, a), __builtin_bit_cast(lbf16x8, b), c, 0, 0, 0);
}

// acc[r] (channel 4 q + r of the tile, pixel p) += sum over the J pairs.  src(tap, cb) = address of the pixel's CB8 vector
// for that pair, or NULL for a zero operand.  bankp = [Jp][16][8] fragment of this (bank, tile).
template <typename T, int K, typename SrcFn>
__device__ __forceinline__ void l_accum(lf32x4& acc, const T* __restrict__ bankp, int J, int Jp, int p, int q, SrcFn src) {
  constexpr int KK = K * K;
  if constexpr (std::is_same<T, float>::value) {
    for (int j = 0; j < J; ++j) {
      const int cb = j / KK, tap = j - cb * KK;
      const float* s = src(tap, cb);
      if (!s) continue;
      float x[8];
      V8<float>::ld(s, x);
      const float* wrow = bankp + ((size_t)j * 16 + 4 * q) * 8;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float w[8];
        V8<float>::ld(wrow + r * 8, w);
        float a = acc[r];
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(x[e], w[e], a);
        acc[r] = a;
      }
    }
  } else {
    // four K-steps per trip: their eight 16-byte loads are in flight together (Jp is a multiple of 16; pairs >= J are zero)
    for (int s4 = 0; s4 < Jp; s4 += 16) {
      uint4 av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = s4 + 4 * u + q;
        const int cb = j / KK, tap = j - cb * KK;
        const T* s = j < J ? src(tap, cb) : nullptr;
        bv[u] = s ? *reinterpret_cast<const uint4*>(s) : make_uint4(0u, 0u, 0u, 0u);
        av[u] = *reinterpret_cast<const uint4*>(bankp + ((size_t)j * 16 + p) * 8);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = l_mfma<std::is_same<T, f16_t>::value>(av[u], bv[u], acc);
    }
  }
}

// ---- frame forward: Y[frame] = bias + W_bank * X --------------------------------------------------
template <typename T, int K>
__global__ __launch_bounds__(256) void k_learned_frame_fwd(LGeom g, const T* __restrict__ X, const T* __restrict__ bank,
                                                           const float* __restrict__ bias, T* __restrict__ Y) {
  const int lane = threadIdx.x & 63, p = lane & 15, q = lane >> 4;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)g.N * g.frame_groups * g.CT) return;                // (uniform per wave)
  const int ct = (int)(item % g.CT);
  const long r0 = item / g.CT;
  int gi = (int)(r0 % g.frame_groups);
  const int n = (int)(r0 / g.frame_groups);
  int b = 0;
  LReg R = l_region(g, 0);
#pragma unroll 1
  for (;;) {
    const int ng = (R.rh * R.rw + 15) / 16;
    if (gi < ng || b == 7) break;
    gi -= ng;
    R = l_region(g, ++b);
  }
  const int pi = gi * 16 + p;
  const bool valid = pi < R.rh * R.rw;
  const int pc = valid ? pi : 0;
  const int ty = pc / R.rw, tx = pc - ty * R.rw;
  const T* xb = X + cb8_index(n, 0, R.sy + ty, R.sx + tx, g.CBin, g.H, g.W);
  const size_t plane = (size_t)g.H * g.W * 8;
  const int W = g.W;
  auto src = [&](int tap, int cb) -> const T* {
    const int dy = tap / K, dx = tap - dy * K;
    return xb + cb * plane + ((size_t)dy * W + dx) * 8;
  };
  lf32x4 acc = {0.f, 0.f, 0.f, 0.f};
  l_accum<T, K>(acc, bank + (size_t)(b * g.CT + ct) * g.Jp * 128, g.J, g.Jp, p, q, src);
  const int co0 = ct * 16 + 4 * q;
  if (valid && co0 < g.CBout * 8) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = co0 + r < g.Cout ? acc[r] + (bias ? bias[co0 + r] : 0.f) : 0.f;
    L4<T>::st(Y + cb8_index(n, co0 >> 3, R.dy + ty, R.dx + tx, g.CBout, g.Ho, g.Wo) + (co0 & 7), v);
  }
}

// ---- frame input gradient: dX[bands] += sum over the banks that read the pixel ---------------------
template <typename T, int K>
__global__ __launch_bounds__(256) void k_learned_frame_dgrad(LGeom g, const T* __restrict__ dY, const T* __restrict__ bank,
                                                             T* __restrict__ dX) {
  const int lane = threadIdx.x & 63, p = lane & 15, q = lane >> 4;
  const int groups = (g.band_pix + 15) / 16;
  const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= (long)g.N * groups * g.IT) return;
  const int it = (int)(item % g.IT);
  const long r0 = item / g.IT;
  const int gi = (int)(r0 % groups);
  const int n = (int)(r0 / groups);
  const int bi = gi * 16 + p;
  const bool valid = bi < g.band_pix;
  const int bc = valid ? bi : 0;
  int iy, ix;
  if (bc < g.nrb * g.W) {
    const int r = bc / g.W;
    ix = bc - r * g.W;
    iy = r < g.pad_y ? r : r + (g.H - g.nrb);
  } else {
    const int t = bc - g.nrb * g.W, r = t / g.ncb, c = t - r * g.ncb;
    iy = g.pad_y + r;
    ix = c < g.pad_x ? c : c + (g.W - g.ncb);
  }
  lf32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int b = 0; b < 8; ++b) {
    const LReg R = l_region(g, b);
    const bool in = valid && iy >= R.sy && iy < R.sy + R.sh && ix >= R.sx && ix < R.sx + R.sw;
    if (!__any(in)) continue;
    // output pixel of tap (dy, dx): (ry - dy, rx - dx) of the bank's rectangle; which taps fall inside it, as bit masks
    const int ry = iy - R.sy, rx = ix - R.sx;
    unsigned rm = 0, cm = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      rm |= (unsigned)(in && ry - t >= 0 && ry - t < R.rh) << t;
      cm |= (unsigned)(rx - t >= 0 && rx - t < R.rw) << t;
    }
    const long base = (long)cb8_index(n, 0, R.dy + ry, R.dx + rx, g.CBout, g.Ho, g.Wo);
    const long plane = (long)g.Ho * g.Wo * 8;
    const int Wo = g.Wo;
    auto src = [&](int tap, int cbo) -> const T* {
      const int dy = tap / K, dx = tap - dy * K;
      if (!((rm >> dy) & (cm >> dx) & 1u)) return nullptr;
      return dY + (base + cbo * plane - (long)(dy * Wo + dx) * 8);
    };
    l_accum<T, K>(acc, bank + (size_t)(b * g.IT + it) * g.Jdp * 128, g.Jd, g.Jdp, p, q, src);
  }
  const int ci0 = it * 16 + 4 * q;
  if (valid && ci0 < g.CBin * 8) {
    T* d = dX + cb8_index(n, ci0 >> 3, iy, ix, g.CBin, g.H, g.W) + (ci0 & 7);
    float v[4];
    L4<T>::ld(d, v);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += acc[r];
    L4<T>::st(d, v);
  }
}

// the waves' register tiles -> one partial slab, summed through LDS in wave order.  acc[tap][r] / bs[r] of lane (cl, q) belong
// to (co = 4 q + r, ci = cl) of the block's (co tile, ci tile).
template <int NWV, int KK, typename Acc, typename Bs>
__device__ __forceinline__ void l_wgrad_store(const LGeom& g, float* __restrict__ ws, int ct, int it, const Acc& acc, const Bs& bs,
                                              float (&red)[NWV][20][64], float (&bred)[NWV][16]) {
  constexpr int RT = 5;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, cl = lane & 15, q = lane >> 4;
  const size_t nW = (size_t)KK * g.CT * g.IT * 256;
  float* slab = ws + (size_t)blockIdx.x * (nW + (size_t)g.CT * 16);
#pragma unroll
  for (int t0 = 0; t0 < KK; t0 += RT) {
#pragma unroll
    for (int tt = 0; tt < RT; ++tt)
      if (t0 + tt < KK) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wv][tt * 4 + r][lane] = acc[t0 + tt][r];
      }
    __syncthreads();
    const int nt = KK - t0 < RT ? KK - t0 : RT;
    for (int e = threadIdx.x; e < nt * 4 * 64; e += 64 * NWV) {
      const int idx = e >> 6, ln = e & 63;
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < NWV; ++w) sum += red[w][idx][ln];
      const int tap = t0 + (idx >> 2), r = idx & 3;
      slab[((((size_t)tap * g.CT + ct) * g.IT + it) * 16 + 4 * (ln >> 4) + r) * 16 + (ln & 15)] = sum;
    }
    __syncthreads();
  }
  if (it == 0) {
    if (cl == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bred[wv][4 * q + r] = bs[r];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      float sum = 0.f;
#pragma unroll
      for (int w = 0; w < NWV; ++w) sum += bred[w][threadIdx.x];
      slab[nW + ct * 16 + threadIdx.x] = sum;
    }
  }
}

// ---- frame filter gradient: partial slabs ----------------------------------------------------------
// One block per (slice, co tile x ci tile).  Lane (cl = input channel, q) of every wave keeps dW[tap][4 q + r][cl] in
// registers; the eight waves take the slice's visits (sample, pixel) round-robin, two at a time so that their loads overlap
// (a visit is 26 loads and 100 FMAs: the kernel is bound by load latency, not by arithmetic), and are summed through LDS in
// wave order.
constexpr int LW_WAVES = 8;
template <typename TX, typename TG, int K>
__global__ __launch_bounds__(64 * LW_WAVES) void k_learned_frame_wgrad(LGeom g, const TX* __restrict__ X, const TG* __restrict__ dY,
                                                                       float* __restrict__ ws, int SL) {
  constexpr int KK = K * K, U = 2, RT = 5;
  __shared__ float red[LW_WAVES][RT * 4][64];
  __shared__ float bred[LW_WAVES][16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, cl = lane & 15, q = lane >> 4;
  const int ct = blockIdx.y / g.IT, it = blockIdx.y - ct * g.IT;
  int ls = blockIdx.x, b = 0;
  LReg R = l_region(g, 0);
  int V = g.N * R.rh * R.rw;
#pragma unroll 1
  for (;;) {
    const int ns = (V + SL - 1) / SL;
    if (ls < ns || b == 7) break;
    ls -= ns;
    R = l_region(g, ++b);
    V = g.N * R.rh * R.rw;
  }
  const int v0 = ls * SL, v1 = v0 + SL < V ? v0 + SL : V;
  const int ci = it * 16 + cl, co0 = ct * 16 + 4 * q;
  const bool xin = ci < g.CBin * 8, gin = co0 < g.CBout * 8;
  const int rpix = R.rh * R.rw;
  float acc[KK][4];
#pragma unroll
  for (int t = 0; t < KK; ++t) { acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.f; }
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int vb = v0 + wv * U; vb < v1; vb += LW_WAVES * U) {
    float d[U][4], x[U][KK];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = vb + u < v1;
      const int v = ok ? vb + u : v1 - 1;
      const int n = v / rpix, rem = v - n * rpix;
      const int ty = rem / R.rw, tx = rem - ty * R.rw;
      d[u][0] = d[u][1] = d[u][2] = d[u][3] = 0.f;
      if (gin && ok) L4<TG>::ld(dY + cb8_index(n, co0 >> 3, R.dy + ty, R.dx + tx, g.CBout, g.Ho, g.Wo) + (co0 & 7), d[u]);
      const TX* xp = X + cb8_index(n, xin ? ci >> 3 : 0, R.sy + ty, R.sx + tx, g.CBin, g.H, g.W) + (ci & 7);
#pragma unroll
      for (int t = 0; t < KK; ++t) {
        const int dy = t / K, dx = t - dy * K;
        x[u][t] = xin ? L4<TX>::ld1(xp + ((size_t)dy * g.W + dx) * 8) : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bs[r] += d[u][r];
#pragma unroll
      for (int t = 0; t < KK; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = fmaf(x[u][t], d[u][r], acc[t][r]);
    }
  }
  l_wgrad_store<LW_WAVES, KK>(g, ws, ct, it, acc, bs, red, bred);
}

// 16-bit types: the same slices and slabs on v_mfma_f32_16x16x32_bf16 with M = 16 output channels, N = 16 input channels
// and K = 32 visits.  An operand lane needs 8 visits of ONE channel, which the CB8 layout keeps 16 bytes apart, so every
// operand is gathered with eight 2-byte loads (a transposing LDS stage would save loads, not arithmetic: at these sizes the
// kernel is bound by the gather).  f16 activations (MC_MIX16) are converted to bf16 on load, as in mc_conv2d_wgrad.  The bias
// sums come from one more MFMA against a fragment of ones.
constexpr int LM_WAVES = 4;
template <bool XH16, int K>
__global__ __launch_bounds__(64 * LM_WAVES) void k_learned_frame_wgrad_mfma(LGeom g, const uint16_t* __restrict__ X,
                                                                            const uint16_t* __restrict__ dY, float* __restrict__ ws, int SL) {
  constexpr int KK = K * K;
  __shared__ float red[LM_WAVES][20][64];
  __shared__ float bred[LM_WAVES][16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
  const int ct = blockIdx.y / g.IT, it = blockIdx.y - ct * g.IT;
  int ls = blockIdx.x, b = 0;
  LReg R = l_region(g, 0);
  int V = g.N * R.rh * R.rw;
#pragma unroll 1
  for (;;) {
    const int ns = (V + SL - 1) / SL;
    if (ls < ns || b == 7) break;
    ls -= ns;
    R = l_region(g, ++b);
    V = g.N * R.rh * R.rw;
  }
  const int v0 = ls * SL, v1 = v0 + SL < V ? v0 + SL : V;
  const int co = ct * 16 + m, ci = it * 16 + m;
  const bool gin = co < g.CBout * 8, xin = ci < g.CBin * 8;
  const int rpix = R.rh * R.rw;
  const size_t HW = (size_t)g.H * g.W, HWo = (size_t)g.Ho * g.Wo;
  lf32x4 acc[KK];
#pragma unroll
  for (int t = 0; t < KK; ++t) acc[t] = (lf32x4){0.f, 0.f, 0.f, 0.f};
  lf32x4 accb = {0.f, 0.f, 0.f, 0.f};
  const uint4 ones = make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
#pragma unroll 1
  for (int vc = v0 + wv * 32; vc < v1; vc += LM_WAVES * 32) {
    // this lane's eight visits vc + 8 q + e: decoded once, then stepped through the bank's output rectangle
    const int vf = vc + 8 * q;
    const int vd = vf < v1 ? vf : v1 - 1;
    int n = vd / rpix;
    const int rem = vd - n * rpix;
    int ty = rem / R.rw, tx = rem - ty * R.rw;
    size_t xo[8];
    uint32_t a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = vf + e < v1;
      const size_t go = ((size_t)(n * g.CBout + (gin ? co >> 3 : 0)) * HWo + (size_t)(R.dy + ty) * g.Wo + (R.dx + tx)) * 8 + (co & 7);
      xo[e] = ((size_t)(n * g.CBin + (xin ? ci >> 3 : 0)) * HW + (size_t)(R.sy + ty) * g.W + (R.sx + tx)) * 8 + (ci & 7);
      a[e] = (gin && ok) ? dY[go] : 0u;                          // (a visit past the slice contributes a zero row)
      if (vf + e + 1 < v1 && ++tx == R.rw) {
        tx = 0;
        if (++ty == R.rh) { ty = 0; ++n; }
      }
    }
    const uint4 av = make_uint4(a[0] | (a[1] << 16), a[2] | (a[3] << 16), a[4] | (a[5] << 16), a[6] | (a[7] << 16));
    accb = l_mfma<false>(av, ones, accb);
#pragma unroll
    for (int t = 0; t < KK; ++t) {
      const int dy = t / K, dx = t - dy * K;
      const size_t off = ((size_t)dy * g.W + dx) * 8;
      uint32_t x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        uint32_t raw = xin ? X[xo[e] + off] : 0u;
        if (XH16) raw = f2bf((float)__builtin_bit_cast(_Float16, (uint16_t)raw));
        x[e] = raw;
      }
      const uint4 bv = make_uint4(x[0] | (x[1] << 16), x[2] | (x[3] << 16), x[4] | (x[5] << 16), x[6] | (x[7] << 16));
      acc[t] = l_mfma<false>(av, bv, acc[t]);
    }
  }
  l_wgrad_store<LM_WAVES, KK>(g, ws, ct, it, acc, accb, red, bred);
}

struct LDw { float* p[8]; };

// dW_unique[bank][u][ci][tap] += sum over the bank's slices of the filter's entry and of its x-mirrored copy's at the
// mirrored tap; dbias[co] += the sum over every slice.  64 outputs per block, the four waves take every fourth slice and are
// combined through LDS; the bias blocks (4 channels each) sum with one lane per slice and a shuffle tree.  Fixed order.
__global__ __launch_bounds__(256) void k_learned_wgrad_reduce(LGeom g, const float* __restrict__ ws, int SL, LDw dw,
                                                              float* __restrict__ db) {
  const int KK = g.KK, K = g.K, CinP = g.IT * 16;
  const size_t nW = (size_t)KK * g.CT * g.IT * 256, slab = nW + (size_t)g.CT * 16;
  const long nOut = (long)8 * KK * g.U * CinP;
  const int nOutBlocks = (int)((nOut + 63) / 64);
  int first[9];
  first[0] = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const LReg R = l_region(g, b);
    first[b + 1] = first[b] + (g.N * R.rh * R.rw + SL - 1) / SL;
  }
  const int e = threadIdx.x & 63, sp = threadIdx.x >> 6;
  if ((int)blockIdx.x >= nOutBlocks) {
    const int co = ((int)blockIdx.x - nOutBlocks) * 4 + sp;
    float s = 0.f;
    if (co < g.Cout)
      for (int k = e; k < first[8]; k += 64) s += ws[(size_t)k * slab + nW + co];
    s = wave_sum(s);
    if (e == 0 && co < g.Cout && db) db[co] += s;
    return;
  }
  __shared__ float red[4][64];
  const long i = (long)blockIdx.x * 64 + e;
  float part = 0.f;
  float* dst = nullptr;
  if (i < nOut) {
    const int cip = (int)(i % CinP);
    long r = i / CinP;
    const int u = (int)(r % g.U); r /= g.U;
    const int tap = (int)(r % KK);
    const int b = (int)(r / KK);
    int s0 = 0, s1 = 0;
    float* d = nullptr;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (k == b) { s0 = first[k]; s1 = first[k + 1]; d = dw.p[k]; }
    if (cip < g.Cin && d) {
      auto at = [&](int t, int co) { return ((((size_t)t * g.CT + (co >> 4)) * g.IT + (cip >> 4)) * 16 + (co & 15)) * 16 + (cip & 15); };
      const size_t o1 = at(tap, u);
      const bool mir = u < g.nh;
      const int ky = tap / K, kx = tap - ky * K;
      const size_t o2 = mir ? at(ky * K + (K - 1 - kx), g.U + u) : o1;
      float a0 = 0.f, a1 = 0.f;
      int k = s0 + sp;
      for (; k + 4 < s1; k += 8) {
        const float* pa = ws + (size_t)k * slab;
        const float* pb = pa + 4 * slab;
        a0 += pa[o1]; a1 += pb[o1];
        if (mir) { a0 += pa[o2]; a1 += pb[o2]; }
      }
      if (k < s1) {
        const float* pa = ws + (size_t)k * slab;
        a0 += pa[o1];
        if (mir) a0 += pa[o2];
      }
      part = a0 + a1;
      dst = d + ((size_t)u * g.Cin + cip) * KK + tap;
    }
  }
  red[sp][e] = part;
  __syncthreads();
  if (sp == 0 && dst) *dst += (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// ---- bank packing (batched over layers) ---------------------------------------------------------------
struct LPkJob {
  int K, Cin, Cout, U, CT, IT, J, Jp, Jd, Jdp, kind_fwd, kind_dg, first_block;   // kind: 0 f32, 1 bf16, 2 f16
  unsigned total_fwd, total;
  const float* w[8];
  void* fwd;
  void* dg;
};
constexpr int LPK_MAX = 16;
struct LPkTable { int n; LPkJob j[LPK_MAX]; };

__device__ __forceinline__ float l_full_weight(const LPkJob& jb, const float* __restrict__ wu, int co, int ci, int tap) {
  if (co >= jb.Cout || ci >= jb.Cin) return 0.f;
  const int K = jb.K, ky = tap / K, kx = tap - ky * K;
  const bool mir = co >= jb.U;
  const int u = mir ? co - jb.U : co, kxs = mir ? K - 1 - kx : kx;
  return wu[(((size_t)u * jb.Cin + ci) * K + ky) * K + kxs];
}
__device__ __forceinline__ void l_store(void* out, size_t i, float v, int kind) {
  if (kind == 0) reinterpret_cast<float*>(out)[i] = v;
  else reinterpret_cast<bf16_t*>(out)[i] = kind == 2 ? __builtin_bit_cast(bf16_t, (_Float16)v) : f2bf(v);
}

__global__ __launch_bounds__(256) void k_learned_pack(LPkTable t) {
  int ji = 0;
#pragma unroll 1
  for (int k = 1; k < t.n; ++k) if ((int)blockIdx.x >= t.j[k].first_block) ji = k;
  const LPkJob& jb = t.j[ji];
  const int nblk = (ji + 1 < t.n ? t.j[ji + 1].first_block : (int)gridDim.x) - jb.first_block;
  const int KK = jb.K * jb.K;
  for (size_t i = (size_t)(blockIdx.x - jb.first_block) * blockDim.x + threadIdx.x; i < jb.total; i += (size_t)nblk * blockDim.x) {
    const bool dgr = i >= jb.total_fwd;
    const size_t l = dgr ? i - jb.total_fwd : i;
    const int e = (int)(l & 7), row = (int)((l >> 3) & 15);
    size_t r = l >> 7;
    const int jp = dgr ? jb.Jdp : jb.Jp, nt = dgr ? jb.IT : jb.CT, jn = dgr ? jb.Jd : jb.J;
    const int j = (int)(r % jp); r /= jp;
    const int tile = (int)(r % nt);
    const int b = (int)(r / nt);
    const float* wu = nullptr;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (k == b) wu = jb.w[k];
    float v = 0.f;
    if (j < jn) {
      const int cb = j / KK, tap = j - cb * KK;
      v = dgr ? l_full_weight(jb, wu, cb * 8 + e, tile * 16 + row, tap) : l_full_weight(jb, wu, tile * 16 + row, cb * 8 + e, tap);
    }
    l_store(dgr ? jb.dg : jb.fwd, l, v, dgr ? jb.kind_dg : jb.kind_fwd);
  }
}

template <typename F> int l_dispatch_k(int K, F f) { return K == 5 ? f(std::integral_constant<int, 5>()) : f(std::integral_constant<int, 3>()); }

}  // namespace

extern "C" {

int32_t mc_learned_validate(const mc_learned_desc* d) {
  LGeom g;
  return l_geom(d, g);
}

size_t mc_learned_bank_bytes(const mc_learned_desc* d, int32_t dgrad) {
  LGeom g;
  if (l_geom(d, g)) return 0;
  return l_bank_elems(g, dgrad) * (g.dtype == MC_F32 ? 4 : 2);
}

size_t mc_learned_wgrad_workspace_bytes(const mc_learned_desc* d) {
  LGeom g;
  if (l_geom(d, g)) return 0;
  int SL, S;
  l_wgrad_plan(g, SL, S);
  return (size_t)S * l_slab_floats(g) * sizeof(float);
}

int mc_learned_pack_banks_batched(const mc_learned_desc* descs, const float* const* w_unique, void* const* fwd_banks,
                                  void* const* dgrad_banks, int32_t n, void* stream) {
  if (!descs || !w_unique || !fwd_banks || n <= 0) return MC_EINVAL;
  for (int base = 0; base < n; base += LPK_MAX) {
    LPkTable t;
    t.n = n - base < LPK_MAX ? n - base : LPK_MAX;
    int blocks = 0;
    for (int k = 0; k < t.n; ++k) {
      LGeom g;
      const int rc = l_geom(&descs[base + k], g);
      if (rc) return rc;
      LPkJob& j = t.j[k];
      for (int b = 0; b < 8; ++b) {
        j.w[b] = w_unique[(size_t)(base + k) * 8 + b];
        if (!j.w[b]) return MC_EINVAL;
      }
      j.fwd = fwd_banks[base + k];
      j.dg = dgrad_banks ? dgrad_banks[base + k] : nullptr;
      if (!j.fwd) return MC_EINVAL;
      j.K = g.K; j.Cin = g.Cin; j.Cout = g.Cout; j.U = g.U; j.CT = g.CT; j.IT = g.IT; j.J = g.J; j.Jp = g.Jp; j.Jd = g.Jd; j.Jdp = g.Jdp;
      j.kind_fwd = g.dtype == MC_F32 ? 0 : (g.dtype == MC_MIX16 ? 2 : 1);      // MC_MIX16: forward banks f16, gradient banks bf16
      j.kind_dg = g.dtype == MC_F32 ? 0 : 1;
      const size_t tf = l_bank_elems(g, 0), td = j.dg ? l_bank_elems(g, 1) : 0;
      if (tf + td > 0xffffffffull) return MC_EUNSUPPORTED;
      j.total_fwd = (unsigned)tf; j.total = (unsigned)(tf + td);
      j.first_block = blocks;
      blocks += (int)((tf + td + 256 * 8 - 1) / (256 * 8));
    }
    hipLaunchKernelGGL(k_learned_pack, dim3(blocks), dim3(256), 0, (hipStream_t)stream, t);
    MC_CHECK_LAUNCH();
  }
  return MC_OK;
}

int mc_learned_frame_fwd(const mc_learned_desc* d, const void* x, const void* bank, const float* bias, void* y, void* stream) {
  LGeom g;
  const int rc = l_geom(d, g);
  if (rc) return rc;
  if (!x || !bank || !y) return MC_EINVAL;
  const long items = (long)g.N * g.frame_groups * g.CT;
  const dim3 grid((unsigned)((items + 3) / 4)), blk(256);
  hipStream_t s = (hipStream_t)stream;
  l_dispatch_k(g.K, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    if (g.dtype == MC_F32) hipLaunchKernelGGL((k_learned_frame_fwd<float, K>), grid, blk, 0, s, g, (const float*)x, (const float*)bank, bias, (float*)y);
    else if (g.dtype == MC_BF16) hipLaunchKernelGGL((k_learned_frame_fwd<bf16_t, K>), grid, blk, 0, s, g, (const bf16_t*)x, (const bf16_t*)bank, bias, (bf16_t*)y);
    else hipLaunchKernelGGL((k_learned_frame_fwd<f16_t, K>), grid, blk, 0, s, g, (const f16_t*)x, (const f16_t*)bank, bias, (f16_t*)y);
    return 0;
  });
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_learned_frame_dgrad(const mc_learned_desc* d, const void* dy, const void* dgrad_bank, void* dx, void* stream) {
  LGeom g;
  const int rc = l_geom(d, g);
  if (rc) return rc;
  if (!dy || !dgrad_bank || !dx) return MC_EINVAL;
  const long items = (long)g.N * ((g.band_pix + 15) / 16) * g.IT;
  const dim3 grid((unsigned)((items + 3) / 4)), blk(256);
  hipStream_t s = (hipStream_t)stream;
  l_dispatch_k(g.K, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    if (g.dtype == MC_F32) hipLaunchKernelGGL((k_learned_frame_dgrad<float, K>), grid, blk, 0, s, g, (const float*)dy, (const float*)dgrad_bank, (float*)dx);
    else hipLaunchKernelGGL((k_learned_frame_dgrad<bf16_t, K>), grid, blk, 0, s, g, (const bf16_t*)dy, (const bf16_t*)dgrad_bank, (bf16_t*)dx);
    return 0;
  });
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_learned_frame_wgrad(const mc_learned_desc* d, const void* x, const void* dy, void* workspace, float* const* dw_unique,
                           float* dbias, void* stream) {
  LGeom g;
  const int rc = l_geom(d, g);
  if (rc) return rc;
  if (!x || !dy || !workspace || !dw_unique) return MC_EINVAL;
  LDw dw;
  for (int b = 0; b < 8; ++b) {
    dw.p[b] = dw_unique[b];
    if (!dw.p[b]) return MC_EINVAL;
  }
  int SL, S;
  l_wgrad_plan(g, SL, S);
  if ((long)g.CT * g.IT > 65535) return MC_EUNSUPPORTED;
  const dim3 grid(S, g.CT * g.IT);
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  l_dispatch_k(g.K, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    if (g.dtype == MC_F32)
      hipLaunchKernelGGL((k_learned_frame_wgrad<float, float, K>), grid, dim3(64 * LW_WAVES), 0, s, g, (const float*)x, (const float*)dy, ws, SL);
    else if (g.dtype == MC_BF16)
      hipLaunchKernelGGL((k_learned_frame_wgrad_mfma<false, K>), grid, dim3(64 * LM_WAVES), 0, s, g, (const uint16_t*)x, (const uint16_t*)dy, ws, SL);
    else
      hipLaunchKernelGGL((k_learned_frame_wgrad_mfma<true, K>), grid, dim3(64 * LM_WAVES), 0, s, g, (const uint16_t*)x, (const uint16_t*)dy, ws, SL);
    return 0;
  });
  MC_CHECK_LAUNCH();
  const long outs = (long)8 * g.KK * g.U * g.IT * 16;
  hipLaunchKernelGGL(k_learned_wgrad_reduce, dim3((unsigned)((outs + 63) / 64 + (g.Cout + 3) / 4)), dim3(256), 0, s, g, (const float*)ws, SL,
                     dw, dbias);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

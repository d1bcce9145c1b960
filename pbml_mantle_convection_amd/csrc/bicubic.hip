// Bicubic resampling over the CB8 layout with host-built tap tables: the tiled and row-walk forward kernels (optionally
// applying the producer's GroupNorm affine + activation on load) and the tiled, row-walk and two-pass adjoints.
#include "common.h"
#include "launch.h"

namespace {

// =================================================================================================
// bicubic resampling with host-built tap tables
// =================================================================================================
// forward: separable.  One block = a 16 x 64 tile of output pixels of one (image, channel block): the input window
// the tile's taps reference (<= 12 x 36 pixels at scale 2) is staged in LDS, filtered along x into a planar f32
// intermediate, then along y.  6.75 vector FMAs and ~0.4 global loads per output instead of 16 and 16.  Outputs whose
// taps leave the window (tables that are not the clamped, monotone bicubic ones) take the direct 16-tap gather.
constexpr int FOH = 16, FOW = 64, FWH = 12, FWW = 36;
template <typename T>
__device__ __forceinline__ void bicubic_direct(const T* __restrict__ x, int n, int cb, int C8, int Hi, int Wi, int yo, int xo,
                                               const int* __restrict__ iy, const float* __restrict__ wy,
                                               const int* __restrict__ ix, const float* __restrict__ wx, float (&acc)[8],
                                               const float* __restrict__ coef4, int act) {
  float sc[8], sh[8];
  if (act >= 0) load_coef8(coef4, n, C8 * 8, cb, sc, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    int ys = iy[yo * 4 + a];
    float wa = wy[yo * 4 + a];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float v[8];
      V8<T>::ld(x + cb8_index(n, cb, ys, ix[xo * 4 + b], C8, Hi, Wi), v);
      if (act >= 0) {
        act_fwd8<FastMath<T>::value>(v, sc, sh, act, v);
        // the staged window holds the activation in the storage type
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = round_storage<T>(v[j]);
      }
      float w = wa * wx[xo * 4 + b];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
    }
  }
}

// one CB8 vector held as raw registers (Q = 1: 8 bf16, Q = 2: 8 f32) -> act(scale * v + shift) in the storage type
template <typename T> struct XformRaw;
template <> struct XformRaw<bf16_t> {
  static __device__ __forceinline__ void apply(uint4 (&r)[1], const float (&sc)[8], const float (&sh)[8], int act) {
    r[0] = xform_bf16x8(r[0], sc, sh, act);
  }
};
template <> struct XformRaw<f16_t> {
  static __device__ __forceinline__ void apply(uint4 (&r)[1], const float (&sc)[8], const float (&sh)[8], int act) {
    r[0] = xform_f16x8(r[0], sc, sh, act);
  }
};
template <> struct XformRaw<float> {
  static __device__ __forceinline__ void apply(uint4 (&r)[2], const float (&sc)[8], const float (&sh)[8], int act) {
    float v[8] = {__uint_as_float(r[0].x), __uint_as_float(r[0].y), __uint_as_float(r[0].z), __uint_as_float(r[0].w),
                  __uint_as_float(r[1].x), __uint_as_float(r[1].y), __uint_as_float(r[1].z), __uint_as_float(r[1].w)};
    act_fwd8<false>(v, sc, sh, act, v);
    r[0] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    r[1] = make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7]));
  }
};

// coef4 / act: x is a raw conv output; the producer's GroupNorm affine + activation are applied while the window is staged
// (act < 0: x is used as it is)
template <typename T>
__global__ __launch_bounds__(256) void k_bicubic_fwd(const T* __restrict__ x, int C8, int Hi, int Wi, int Ho, int Wo,
                                                     const int* __restrict__ iy, const float* __restrict__ wy,
                                                     const int* __restrict__ ix, const float* __restrict__ wx,
                                                     T* __restrict__ out, int tiles_x, const float* __restrict__ coef4,
                                                     int act) {
  __shared__ __attribute__((aligned(16))) T win[FWH * FWW * 8];
  __shared__ float4 tmp[2][FWH][FOW];
  const int n = blockIdx.z, cb = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * FOH, tx0 = (blockIdx.x % tiles_x) * FOW;
  const int ylo = iy[ty0 * 4], xlo = ix[tx0 * 4];            // clamped bicubic tables are non-decreasing
  {
    constexpr int VPT = (FWH * FWW + 255) / 256, Q = sizeof(T) == 4 ? 2 : 1;
    uint4 rv[VPT][Q];
#pragma unroll
    for (int m = 0; m < VPT; ++m) {
      int i = min((int)threadIdx.x + m * 256, FWH * FWW - 1);
      int r = i / FWW, c = i - r * FWW;
      const T* p = x + cb8_index(n, cb, min(ylo + r, Hi - 1), min(xlo + c, Wi - 1), C8, Hi, Wi);
#pragma unroll
      for (int q = 0; q < Q; ++q) rv[m][q] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p) + 16 * q);
    }
    if (act >= 0) {
      float sc[8], sh[8];
      load_coef8(coef4, n, C8 * 8, cb, sc, sh);
#pragma unroll
      for (int m = 0; m < VPT; ++m) XformRaw<T>::apply(rv[m], sc, sh, act);
    }
#pragma unroll
    for (int m = 0; m < VPT; ++m) {
      int i = threadIdx.x + m * 256;
      if (i < FWH * FWW)
#pragma unroll
        for (int q = 0; q < Q; ++q) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(&win[i * 8]) + 16 * q) = rv[m][q];
    }
  }
  const int lx = threadIdx.x & 63, xo = min(tx0 + lx, Wo - 1);
  int jx[4];
  float fx[4];
  bool xin = true;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    jx[b] = ix[xo * 4 + b] - xlo;
    fx[b] = wx[xo * 4 + b];
    xin = xin && jx[b] >= 0 && jx[b] < FWW;
    jx[b] = min(max(jx[b], 0), FWW - 1);
  }
  __syncthreads();
  // x pass
#pragma unroll
  for (int m = 0; m < FWH / 4; ++m) {
    int r = (threadIdx.x >> 6) + 4 * m;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float v[8];
      V8<T>::ld(&win[(r * FWW + jx[b]) * 8], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += fx[b] * v[j];
    }
    tmp[0][r][lx] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    tmp[1][r][lx] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
  __syncthreads();
  // y pass
#pragma unroll
  for (int k = 0; k < FOH / 4; ++k) {
    int yo = ty0 + (threadIdx.x >> 6) + 4 * k;
    if (yo >= Ho || tx0 + lx >= Wo) continue;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool fast = xin;
    int jy[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      jy[a] = iy[yo * 4 + a] - ylo;
      fast = fast && jy[a] >= 0 && jy[a] < FWH;
    }
    if (fast) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        float wa = wy[yo * 4 + a];
        float4 p0 = tmp[0][jy[a]][lx], p1 = tmp[1][jy[a]][lx];
        acc[0] += wa * p0.x; acc[1] += wa * p0.y; acc[2] += wa * p0.z; acc[3] += wa * p0.w;
        acc[4] += wa * p1.x; acc[5] += wa * p1.y; acc[6] += wa * p1.z; acc[7] += wa * p1.w;
      }
    } else {
      bicubic_direct<T>(x, n, cb, C8, Hi, Wi, yo, xo, iy, wy, ix, wx, acc, coef4, act);
    }
    V8<T>::st(out + cb8_index(n, cb, yo, xo, C8, Ho, Wo), acc);
  }
}

// The upsample as a walk down the output rows (the forward twin of k_bicubic_bwd_walk below): thread = output column of a
// strip, block = strip x chunk of output rows of one (sample, channel block).  An input row crosses LDS once (storage type,
// activated on the way if asked), every thread interpolates it along x into registers (f32), and a register window of the
// four x-interpolated rows under the current output row slides with the first tap; an output row is 4 x 8 FMAs and one
// coalesced 16-byte store per thread.  Same summation order as the tiled kernel (x taps, then y taps) on unclamped rows.
template <typename T, int SW>
__global__ __launch_bounds__(SW) void k_bicubic_fwd_walk(const T* __restrict__ x, int C8, int Hi, int Wi, int Ho, int Wo,
                                                         const int* __restrict__ iy, const float* __restrict__ wy,
                                                         const int* __restrict__ ix, const float* __restrict__ wx,
                                                         T* __restrict__ out, int rpc, int fw, int strips,
                                                         const float* __restrict__ coef4, int act) {
  constexpr int Q = sizeof(T) == 4 ? 2 : 1;
  __shared__ uint4 crow[2][Q][SW];
  const int n = blockIdx.z, cb = blockIdx.y, c = threadIdx.x;
  const int strip = blockIdx.x % strips, chunk = blockIdx.x / strips;
  const int r0 = chunk * rpc, r1 = min(Ho, r0 + rpc);
  const int F0 = strip * fw, F1 = min(Wo, F0 + fw);
  if (r0 >= r1 || F0 >= F1) return;                                     // (block-uniform)
  const int C0 = ix[F0 * 4];                                            // clamped tables are non-decreasing
  const int ncw = min(ix[(F1 - 1) * 4 + 3] - C0 + 1, SW);
  const bool outok = F0 + c < F1;
  const int xo = min(F0 + c, F1 - 1);
  int jx[4];
  float fx[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    jx[b] = min(max(ix[xo * 4 + b] - C0, 0), SW - 1);
    fx[b] = wx[xo * 4 + b];
  }
  float sc[8], sh[8];
  if (act >= 0) load_coef8(coef4, n, C8 * 8, cb, sc, sh);
  const T* src = x + cb8_index(n, cb, 0, min(C0 + c, Wi - 1), C8, Hi, Wi);
  const size_t rstride = (size_t)Wi * 8;
  auto ldrow = [&](int yi, uint4 (&r)[Q]) {
    if (c < ncw) {
      const char* p = reinterpret_cast<const char*>(src + (size_t)min(yi, Hi - 1) * rstride);
#pragma unroll
      for (int q = 0; q < Q; ++q) r[q] = *reinterpret_cast<const uint4*>(p + 16 * q);
    }
  };
  float win[4][8];
  int buf = 0;
  // input row (registers) -> LDS -> this thread's x interpolation, into the top of the window
  auto push = [&](uint4 (&r)[Q]) {
    if (c < ncw) {
      if (act >= 0) XformRaw<T>::apply(r, sc, sh, act);
#pragma unroll
      for (int q = 0; q < Q; ++q) crow[buf][q][c] = r[q];
    }
    __syncthreads();                       // (one barrier per input row: the buffer written two rows on was read before the next one)
#pragma unroll
    for (int j = 0; j < 8; ++j) { win[0][j] = win[1][j]; win[1][j] = win[2][j]; win[2][j] = win[3][j]; win[3][j] = 0.f; }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      float v[8];
      if constexpr (sizeof(T) == 4) {
        const uint4 lo = crow[buf][0][jx[b]], hi = crow[buf][Q - 1][jx[b]];
        v[0] = __uint_as_float(lo.x); v[1] = __uint_as_float(lo.y); v[2] = __uint_as_float(lo.z); v[3] = __uint_as_float(lo.w);
        v[4] = __uint_as_float(hi.x); v[5] = __uint_as_float(hi.y); v[6] = __uint_as_float(hi.z); v[7] = __uint_as_float(hi.w);
      } else {
        V8<T>::ld(reinterpret_cast<const T*>(&crow[buf][0][jx[b]]), v);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) win[3][j] += fx[b] * v[j];
    }
    buf ^= 1;
  };
  int basey = __builtin_amdgcn_readfirstlane(iy[r0 * 4]);               // window = input rows basey .. basey + 3 (clamped)
  uint4 nx[Q];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ldrow(basey + k, nx);
    push(nx);
  }
  ldrow(basey + 4, nx);                                                  // the next row: in flight until the window slides
  for (int yo = r0; yo < r1; ++yo) {
    const int t0 = __builtin_amdgcn_readfirstlane(iy[yo * 4]), t1 = __builtin_amdgcn_readfirstlane(iy[yo * 4 + 1]),
              t2 = __builtin_amdgcn_readfirstlane(iy[yo * 4 + 2]), t3 = __builtin_amdgcn_readfirstlane(iy[yo * 4 + 3]);
    const float w0 = wy[yo * 4], w1 = wy[yo * 4 + 1], w2 = wy[yo * 4 + 2], w3 = wy[yo * 4 + 3];
    while (basey < t0) {
      push(nx);
      ++basey;
      ldrow(basey + 4, nx);
    }
    float o[8];
    if (t1 == basey + 1 && t2 == basey + 2 && t3 == basey + 3) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float a = w0 * win[0][j];
        a += w1 * win[1][j]; a += w2 * win[2][j]; a += w3 * win[3][j];
        o[j] = a;
      }
    } else {                                                             // clamped taps: several read one row
      const int q1 = t1 - basey, q2 = t2 - basey, q3 = t3 - basey;
      float wk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) wk[k] = (k == 0 ? w0 : 0.f) + (q1 == k ? w1 : 0.f) + (q2 == k ? w2 : 0.f) + (q3 == k ? w3 : 0.f);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = wk[0] * win[0][j] + wk[1] * win[1][j] + wk[2] * win[2][j] + wk[3] * win[3][j];
    }
    if (outok) V8<T>::st(out + cb8_index(n, cb, yo, xo, C8, Ho, Wo), o);
  }
}

// adjoint of the bicubic upsample, separable.  One block = a 16 x 16 tile of input (low-res) pixels of one channel block:
// the (folded) output-gradient window the tile touches (<= 40 x 40) is staged in LDS in the storage type, reduced along
// y with the transposed tap lists (lanes run over window columns: conflict-free), then along x from a planar f32
// intermediate.  Pixels whose lists leave the window (image borders of large scale factors) gather from global memory.
constexpr int BT = 16, BWIN = 40;
// BYT / BXT: tap-list lengths held on chip (8 covers every list of an even x2 upsample, 12 the odd sizes; longer lists take
// the per-pixel gather path).  With 12 slots for 8-entry lists a third of both passes multiplied zeros (331 us at level 0).
template <typename T, int BYT, int BXT>
__global__ __launch_bounds__(256) void k_bicubic_bwd(mc_grad_src g, int C8, int Hi, int Wi, const int* __restrict__ tys,
                                                     const int* __restrict__ tyj, const float* __restrict__ tyw,
                                                     const int* __restrict__ txs, const int* __restrict__ txj,
                                                     const float* __restrict__ txw, T* __restrict__ dx, int tiles_x, int tiles) {
  __shared__ __attribute__((aligned(16))) T win[BWIN * BWIN * 8];
  __shared__ float4 tmp[2][BT][BWIN];
  __shared__ int s_yj[BT][BYT];
  __shared__ float s_yw[BT][BYT];
  const int n = blockIdx.z, cb = blockIdx.y;
  constexpr int VPT = (BWIN * BWIN + 255) / 256, Q = sizeof(T) == 4 ? 2 : 1;
  const int pad = g.kind == MC_GSRC_PLAIN ? 0 : g.pad;
  const int hs = g.hs + 2 * pad, ws = g.ws + 2 * pad;
  const T* base = reinterpret_cast<const T*>(g.ptr);
  // Round 3: blocks are PERSISTENT over the tiles of their (sample, channel block) and the raw window of tile t + 1 is in
  // flight (registers) while tile t runs its two passes: one block per tile exposed the load latency once per tile with only
  // three blocks resident per CU (45 KB of LDS each).
  uint4 rv[VPT][Q];
  auto window_origin = [&](int tile, int& ty0, int& tx0, int& ylo, int& xlo) {
    ty0 = (tile / tiles_x) * BT; tx0 = (tile % tiles_x) * BT;
    // output ranges referenced by this tile: the transposed tap lists are sorted by output index and monotone in the
    // input index, so the range starts at the first entry of the first row's list (uniform scalar loads)
    ylo = tyj[tys[ty0]]; xlo = txj[txs[tx0]];
  };
  auto load_window = [&](int ylo, int xlo) {
#pragma unroll
    for (int m = 0; m < VPT; ++m) {
      int i = threadIdx.x + m * 256;
      int r = i / BWIN, c = i - r * BWIN;
      bool ok = i < BWIN * BWIN && ylo + r < g.hs && xlo + c < g.ws;
      const T* p = base + cb8_index(n, cb + (g.c8_total > 0 ? g.cb_off : 0), min(ylo + r, g.hs - 1) + pad, min(xlo + c, g.ws - 1) + pad,
                                  g.c8_total > 0 ? g.c8_total : C8, hs, ws);
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        uint4 v = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p) + 16 * q);
        rv[m][q] = ok ? v : make_uint4(0, 0, 0, 0);
      }
    }
  };
  int tile = blockIdx.x;
  if (tile >= tiles) return;
  int ty0, tx0, ylo, xlo;
  window_origin(tile, ty0, tx0, ylo, xlo);
  load_window(ylo, xlo);
  for (; tile < tiles; tile += gridDim.x) {
    const int ty1 = min(ty0 + BT, Hi), tx1 = min(tx0 + BT, Wi);
    // ---- the y tap lists, this thread's x taps, the staged window -> LDS
    if (threadIdx.x < BT * BYT) {
      int ly = threadIdx.x / BYT, k = threadIdx.x - ly * BYT;
      int yi = min(ty0 + ly, Hi - 1);
      int a0 = tys[yi], cnt = tys[yi + 1] - a0;
      int r = k < cnt ? tyj[a0 + k] - ylo : -1;
      bool live = r >= 0 && r < BWIN;                       // dead / out-of-window entries: weight 0 (branch-free passes);
      s_yj[ly][k] = live ? r : 0;                           // pixels with out-of-window entries take the slow path
      s_yw[ly][k] = live ? tyw[a0 + k] : 0.f;
    }
#pragma unroll
    for (int m = 0; m < VPT; ++m) {
      int i = threadIdx.x + m * 256;
      if (i < BWIN * BWIN)
#pragma unroll
        for (int q = 0; q < Q; ++q) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(&win[i * 8]) + 16 * q) = rv[m][q];
    }
    const int ly = threadIdx.x / BT, lx = threadIdx.x % BT;                            // x pass: one thread per pixel
    const int yi = min(ty0 + ly, Hi - 1), xi = min(tx0 + lx, Wi - 1);
    const int a0 = tys[yi], a1 = tys[yi + 1], b0 = txs[xi], nb = txs[xi + 1] - b0;
    int xj[BXT];
    float xw[BXT];
#pragma unroll
    for (int k = 0; k < BXT; ++k) {
      xj[k] = k < nb ? txj[b0 + k] - xlo : 0;
      xw[k] = k < nb ? txw[b0 + k] : 0.f;
    }
    bool fast = a1 - a0 <= BYT && nb <= BXT && (a1 == a0 || (tyj[a0] - ylo >= 0 && tyj[a1 - 1] - ylo < BWIN));
#pragma unroll
    for (int k = 0; k < BXT; ++k) {
      fast = fast && xj[k] >= 0 && xj[k] < BWIN;
      xj[k] = min(max(xj[k], 0), BWIN - 1);
    }
    __syncthreads();
    // the next tile's window: in flight during both passes
    const int cty0 = ty0, ctx0 = tx0;
    if (tile + (int)gridDim.x < tiles) {
      window_origin(tile + gridDim.x, ty0, tx0, ylo, xlo);
      load_window(ylo, xlo);
    }
    // y pass: tmp[ly][c] = sum_a w_a win[yo_a - ylo][c]
    for (int i = threadIdx.x; i < BT * BWIN; i += 256) {
      int py = i / BWIN, c = i - py * BWIN;
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < BYT; ++k) {
        int r = s_yj[py][k];
        float wa = s_yw[py][k];
        float v[8];
        V8<T>::ld(&win[(r * BWIN + c) * 8], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += wa * v[j];
      }
      tmp[0][py][c] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      tmp[1][py][c] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    __syncthreads();
    if (cty0 + ly < ty1 && ctx0 + lx < tx1) {
      float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (fast) {
#pragma unroll
        for (int k = 0; k < BXT; ++k) {                         // dead entries: index 0, weight 0
          float w = xw[k];
          float4 p0 = tmp[0][ly][xj[k]], p1 = tmp[1][ly][xj[k]];
          acc[0] += w * p0.x; acc[1] += w * p0.y; acc[2] += w * p0.z; acc[3] += w * p0.w;
          acc[4] += w * p1.x; acc[5] += w * p1.y; acc[6] += w * p1.z; acc[7] += w * p1.w;
        }
      } else {
        for (int a = a0; a < a1; ++a) {
          int yo = tyj[a];
          float wa = tyw[a];
          for (int b = b0; b < b0 + nb; ++b) {
            float w = wa * txw[b];
            float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            grad_fetch_add<T>(g, n, cb, yo, txj[b], C8, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
          }
        }
      }
      V8<T>::st(dx + cb8_index(n, cb, yi, xi, C8, Hi, Wi), acc);
    }
    __syncthreads();                                       // tmp / win / the tap lists are rewritten by the next tile
  }
}

// The same adjoint as a WALK down the output (high-res) rows: a block owns a strip of SW output columns of one (sample,
// channel block) and a chunk of input rows; thread = output column.  Each output row is read ONCE, straight from global
// memory into registers (two rows in flight), and scattered with the forward taps (4 per row, block-uniform) into a register
// window of the four input rows that are still open; the window slides when the first tap moves on, and the row that
// leaves it is complete in y: it crosses LDS once (f32, even / odd columns apart: conflict-free both ways) and every thread
// pair gathers one input pixel's x taps from it.  Against the tiled kernel above this reads the gradient 1.1 x instead of
// 1.6 x (6 extra rows per chunk, no column halo at <= 512 columns), moves 320 B instead of 760 B through LDS per input
// pixel, and needs about half the instructions.  Any upsample ratio >= 1 in y (the window follows the table); x tap lists
// of <= BXT entries.  Rows whose taps are clamped (image border) take a select form of the same scatter.
template <typename T, int BXT, int SW>
__global__ __launch_bounds__(SW) void k_bicubic_bwd_walk(mc_grad_src g, int C8, int Hi, int Wi, const int* __restrict__ iy,
                                                         const float* __restrict__ wy, const int* __restrict__ tys,
                                                         const int* __restrict__ tyj, const int* __restrict__ txs,
                                                         const int* __restrict__ txj, const float* __restrict__ txw,
                                                         T* __restrict__ dx, int rpc, int cw, int strips) {
  constexpr int PL = SW + 8, ODD = SW / 2 + 8, Q = sizeof(T) == 4 ? 2 : 1;
  __shared__ float4 trow[2][2][PL];
  const int n = blockIdx.z, cb = blockIdx.y, c = threadIdx.x;
  const int strip = blockIdx.x % strips, chunk = blockIdx.x / strips;
  const int m0 = chunk * rpc, m1 = min(Hi, m0 + rpc);
  const int X0 = strip * cw, X1 = min(Wi, X0 + cw);
  if (m0 >= m1 || X0 >= X1) return;                                    // (block-uniform)
  const int F0 = txj[txs[X0]];                                         // first output column this strip's pixels gather from
  const int pad = g.kind == MC_GSRC_PLAIN ? 0 : g.pad;
  const int hs = g.hs + 2 * pad, ws = g.ws + 2 * pad;
  const bool colok = F0 + c < g.ws;
  const T* col = reinterpret_cast<const T*>(g.ptr) + cb8_index(n, cb + (g.c8_total > 0 ? g.cb_off : 0), pad, min(F0 + c, g.ws - 1) + pad,
                                                               g.c8_total > 0 ? g.c8_total : C8, hs, ws);
  const size_t rstride = (size_t)ws * 8;
  // this thread's half pixel of the x pass: input column X0 + c / 2, channels 4 (c & 1) .. + 3
  const int Xc = X0 + (c >> 1), half = c & 1;
  const bool act = Xc < X1;
  int xs[BXT];
  float xw[BXT];
  {
    const int Xq = min(Xc, Wi - 1), b0 = txs[Xq], nb = txs[Xq + 1] - b0;
#pragma unroll
    for (int k = 0; k < BXT; ++k) {
      int j = k < nb ? txj[b0 + k] - F0 : 0;
      j = min(max(j, 0), SW - 1);
      xs[k] = (j >> 1) + (j & 1) * ODD;
      xw[k] = k < nb ? txw[b0 + k] : 0.f;
    }
  }
  const int myslot = (c >> 1) + (c & 1) * ODD;
  const int fs = __builtin_amdgcn_readfirstlane(tyj[tys[m0]]), fe = __builtin_amdgcn_readfirstlane(tyj[tys[m1] - 1]);
  int basey = __builtin_amdgcn_readfirstlane(iy[fs * 4]);
  float acc[4][8];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
  int buf = 0;
  auto ldrow = [&](int yo, uint4 (&r)[Q]) {
    const char* p = reinterpret_cast<const char*>(col + (size_t)yo * rstride);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      uint4 v = *reinterpret_cast<const uint4*>(p + 16 * q);
      r[q] = colok ? v : make_uint4(0, 0, 0, 0);
    }
  };
  // the oldest open input row is complete: x pass (if it is one of this chunk's rows), then the window slides
  auto emit = [&]() {
    if (basey >= m0 && basey < m1) {
      trow[buf][0][myslot] = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
      trow[buf][1][myslot] = make_float4(acc[0][4], acc[0][5], acc[0][6], acc[0][7]);
      __syncthreads();                     // (one barrier per row: the buffer written two rows on was read before the next one)
      if (act) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < BXT; ++k) {                                 // dead entries: slot 0, weight 0
          const float4 p = trow[buf][half][xs[k]];
          o.x += xw[k] * p.x; o.y += xw[k] * p.y; o.z += xw[k] * p.z; o.w += xw[k] * p.w;
        }
        T* d = dx + cb8_index(n, cb, basey, Xc, C8, Hi, Wi) + 4 * half;
        if constexpr (sizeof(T) == 4) *reinterpret_cast<float4*>(d) = o;
        else *reinterpret_cast<uint2*>(d) = make_uint2(pk_bf16(o.x, o.y), pk_bf16(o.z, o.w));
      }
      buf ^= 1;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { acc[0][j] = acc[1][j]; acc[1][j] = acc[2][j]; acc[2][j] = acc[3][j]; acc[3][j] = 0.f; }
    ++basey;
  };
  uint4 p0[Q], p1[Q];
  ldrow(fs, p0);
  ldrow(min(fs + 1, fe), p1);
  for (int yo = fs; yo <= fe; ++yo) {
    uint4 cur[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) { cur[q] = p0[q]; p0[q] = p1[q]; }
    if (yo + 2 <= fe) ldrow(yo + 2, p1);
    const int t0 = __builtin_amdgcn_readfirstlane(iy[yo * 4]), t1 = __builtin_amdgcn_readfirstlane(iy[yo * 4 + 1]),
              t2 = __builtin_amdgcn_readfirstlane(iy[yo * 4 + 2]), t3 = __builtin_amdgcn_readfirstlane(iy[yo * 4 + 3]);
    const float w0 = wy[yo * 4], w1 = wy[yo * 4 + 1], w2 = wy[yo * 4 + 2], w3 = wy[yo * 4 + 3];
    while (basey < t0) emit();
    float v[8];
    if constexpr (sizeof(T) == 4) {
      v[0] = __uint_as_float(cur[0].x); v[1] = __uint_as_float(cur[0].y); v[2] = __uint_as_float(cur[0].z); v[3] = __uint_as_float(cur[0].w);
      v[4] = __uint_as_float(cur[Q - 1].x); v[5] = __uint_as_float(cur[Q - 1].y); v[6] = __uint_as_float(cur[Q - 1].z); v[7] = __uint_as_float(cur[Q - 1].w);
    } else {
      v[0] = __uint_as_float(cur[0].x << 16); v[1] = __uint_as_float(cur[0].x & 0xffff0000u);
      v[2] = __uint_as_float(cur[0].y << 16); v[3] = __uint_as_float(cur[0].y & 0xffff0000u);
      v[4] = __uint_as_float(cur[0].z << 16); v[5] = __uint_as_float(cur[0].z & 0xffff0000u);
      v[6] = __uint_as_float(cur[0].w << 16); v[7] = __uint_as_float(cur[0].w & 0xffff0000u);
    }
    if (t1 == basey + 1 && t2 == basey + 2 && t3 == basey + 3) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { acc[0][j] += w0 * v[j]; acc[1][j] += w1 * v[j]; acc[2][j] += w2 * v[j]; acc[3][j] += w3 * v[j]; }
    } else {                                                             // clamped taps: several land on one row
      const int r1 = t1 - basey, r2 = t2 - basey, r3 = t3 - basey;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float wk = (k == 0 ? w0 : 0.f) + (r1 == k ? w1 : 0.f) + (r2 == k ? w2 : 0.f) + (r3 == k ? w3 : 0.f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] += wk * v[j];
      }
    }
  }
#pragma unroll 1
  for (int k = 0; k < 4; ++k) emit();
}

// (Round 3 tried a streaming form -- wave = input row, lanes over the output columns, the row's transposed tap list summed
// straight from global memory, then an x pass from one f32 row in LDS: +0.12 ms per step.  Every output row is read by the
// four input rows it feeds, and those re-reads come from L2, not from the 16 KB L1: 4 x the bytes cross the L2 -> CU path.
// The LDS window above is the right structure; what it costs is reading the window 8 + 8 times through LDS.)
// adjoint of the bicubic upsample for LARGE scale factors (NewFluidNet: x4, x8, x16), where the tile window of the kernel
// above does not fit and its per-pixel fallback gathers taps_y x taps_x (up to 64 x 64) vectors: two 1-D passes through an
// f32 intermediate [n][c8][hi][wo][8] instead (taps_y + taps_x per pixel, coalesced along x).
template <typename T>
__global__ void k_bicubic_bwd_ypass(mc_grad_src g, int C8, int Hi, int Wo, const int* __restrict__ tys,
                                    const int* __restrict__ tyj, const float* __restrict__ tyw, float* __restrict__ tmp) {
  const int n = blockIdx.z, cb = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hi * Wo; i += gridDim.x * blockDim.x) {
    const int yi = i / Wo, xo = i - yi * Wo;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = tys[yi]; a < tys[yi + 1]; ++a) {
      float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      grad_fetch_add<T>(g, n, cb, tyj[a], xo, C8, v);
      const float w = tyw[a];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
    }
    V8<float>::st(tmp + cb8_index(n, cb, yi, xo, C8, Hi, Wo), acc);
  }
}
template <typename T>
__global__ void k_bicubic_bwd_xpass(const float* __restrict__ tmp, int C8, int Hi, int Wi, int Wo, const int* __restrict__ txs,
                                    const int* __restrict__ txj, const float* __restrict__ txw, T* __restrict__ dx) {
  const int n = blockIdx.z, cb = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hi * Wi; i += gridDim.x * blockDim.x) {
    const int yi = i / Wi, xi = i - yi * Wi;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = txs[xi]; b < txs[xi + 1]; ++b) {
      float v[8];
      V8<float>::ld(tmp + cb8_index(n, cb, yi, txj[b], C8, Hi, Wo), v);
      const float w = txw[b];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
    }
    V8<T>::st(dx + cb8_index(n, cb, yi, xi, C8, Hi, Wi), acc);
  }
}

}  // namespace

extern "C" {

int mc_bicubic_fwd_act(const void* x, const float* coef, int32_t act, int32_t n, int32_t c, int32_t hi, int32_t wi,
                       int32_t ho, int32_t wo, const int32_t* idx_y, const float* wgt_y, const int32_t* idx_x,
                       const float* wgt_x, int32_t dtype, void* out, void* stream) {
  if (!x || !out || !idx_y || !wgt_y || !idx_x || !wgt_x || n <= 0 || c <= 0 || hi <= 0 || wi <= 0 || ho <= 0 || wo <= 0)
    return MC_EINVAL;
  if (act < MC_ACT_NONE || act > MC_ACT_ELU) return MC_EINVAL;
  const int a = (coef == nullptr && act == MC_ACT_NONE) ? -1 : act;      // -1: x is used as it is
  int C8 = (c + 7) / 8;
  hipStream_t s = (hipStream_t)stream;
  static const int walk = env_int("MC_BICUBIC_FWD_WALK", 1);
  if (walk && ho >= hi && wo >= wi) {                                    // upsampling: the row walk (taps span <= 4 rows / 4 columns)
    const int SW = wo <= 128 ? 128 : (wo <= 256 ? 256 : 512);
    // one strip when the output row fits the block; else strips of SW - 8 output columns (their input span <= SW - 4)
    const int fw = wo <= SW ? wo : SW - 8, strips = cdiv(wo, fw);
    static const int target = env_int("MC_BICUBIC_FWD_WALK_BLOCKS", 1024);
    const int chunks = max(1, min(cdiv(target, C8 * n * strips), cdiv(ho, 8)));
    const int rpc = cdiv(ho, chunks);
    dim3 g(cdiv(ho, rpc) * strips, C8, n);
    return with_storage_type(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, dim3(SW), 0, s, (const T*)x, C8, hi, wi, ho, wo, idx_y, wgt_y, idx_x, wgt_x, (T*)out, rpc, fw, strips, coef, a); };
      if (SW == 128) launch(k_bicubic_fwd_walk<T, 128>); else if (SW == 256) launch(k_bicubic_fwd_walk<T, 256>); else launch(k_bicubic_fwd_walk<T, 512>);
    });
  }
  int tiles_x = cdiv(wo, FOW), tiles_y = cdiv(ho, FOH);
  dim3 g(tiles_x * tiles_y, C8, n);
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_bicubic_fwd<T>, g, dim3(256), 0, s, (const T*)x, C8, hi, wi, ho, wo, idx_y, wgt_y, idx_x, wgt_x, (T*)out, tiles_x, coef, a);
  });
}

int mc_bicubic_fwd(const void* x, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                   const int32_t* idx_y, const float* wgt_y, const int32_t* idx_x, const float* wgt_x, int32_t dtype,
                   void* out, void* stream) {
  return mc_bicubic_fwd_act(x, nullptr, MC_ACT_NONE, n, c, hi, wi, ho, wo, idx_y, wgt_y, idx_x, wgt_x, dtype, out, stream);
}

int mc_bicubic_bwd_taps(const mc_grad_src* gs, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                        const int32_t* tys, const int32_t* tyj, const float* tyw, const int32_t* txs, const int32_t* txj,
                        const float* txw, int32_t max_taps_y, int32_t max_taps_x, int32_t dtype, void* dx, void* stream) {
  if (!gs || !dx || !tys || !tyj || !tyw || !txs || !txj || !txw || n <= 0 || c <= 0) return MC_EINVAL;
  int rc = check_gsrc(gs);
  if (rc) return rc;
  if (gs->hs != ho || gs->ws != wo) return MC_EINVAL;
  if (gs->kind != MC_GSRC_PLAIN && gs->kind != MC_GSRC_PADFOLD) return MC_EUNSUPPORTED;   // the window is staged raw
  int C8 = (c + 7) / 8;
  hipStream_t s = (hipStream_t)stream;
  int tiles_x = cdiv(wi, BT), tiles_y = cdiv(hi, BT);
  // persistent blocks: ~6 resident per CU over the (tile, channel block, sample) grid, several tiles each
  static const int per_cu = env_int("MC_BICUBIC_BLOCKS_PER_CU", 6);
  const int want = max(1, (256 * per_cu) / max(1, C8 * n));
  dim3 g(min(tiles_x * tiles_y, want), C8, n);
  const bool y8 = max_taps_y > 0 && max_taps_y <= 8, x8 = max_taps_x > 0 && max_taps_x <= 8;
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, *gs, C8, hi, wi, tys, tyj, tyw, txs, txj, txw, (T*)dx, tiles_x, tiles_x * tiles_y); };
    if (y8 && x8) launch(k_bicubic_bwd<T, 8, 8>); else if (y8) launch(k_bicubic_bwd<T, 8, 12>); else if (x8) launch(k_bicubic_bwd<T, 12, 8>); else launch(k_bicubic_bwd<T, 12, 12>);
  });
}

int mc_bicubic_bwd_walk(const mc_grad_src* gs, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                        const int32_t* idx_y, const float* wgt_y, const int32_t* tys, const int32_t* tyj, const int32_t* txs,
                        const int32_t* txj, const float* txw, int32_t max_taps_x, int32_t dtype, void* dx, void* stream) {
  if (!gs || !dx || !idx_y || !wgt_y || !tys || !tyj || !txs || !txj || !txw || n <= 0 || c <= 0) return MC_EINVAL;
  int rc = check_gsrc(gs);
  if (rc) return rc;
  if (gs->hs != ho || gs->ws != wo || hi <= 0 || wi <= 0 || ho < hi || wo < wi) return MC_EINVAL;
  if (gs->kind != MC_GSRC_PLAIN && gs->kind != MC_GSRC_PADFOLD) return MC_EUNSUPPORTED;   // rows are read raw
  if (max_taps_x <= 0 || max_taps_x > 12) return MC_EUNSUPPORTED;
  const int C8 = (c + 7) / 8;
  hipStream_t s = (hipStream_t)stream;
  const int SW = wo <= 128 ? 128 : (wo <= 256 ? 256 : 512);
  // one strip when the row fits the block; else strips of cw input columns whose taps span <= SW output columns:
  // input column X gathers from output columns [s (X - 1.5) - 0.5, s (X + 2.5) - 0.5), s = wo / wi
  int cw = wi, strips = 1;
  if (wo > SW || wi > SW / 2) {
    cw = min(SW / 2, (int)((int64_t)(SW - 1) * wi / wo) - 3);
    if (cw < 1) return MC_EUNSUPPORTED;
    strips = cdiv(wi, cw);
  }
  static const int target = env_int("MC_BICUBIC_WALK_BLOCKS", 1024);   // (in-step A/B, 256 / 512 / 1024 / 2048 / 4096: +0.08 / 0 / -0.04 / -0.02 / +0.03 ms)
  const int chunks = max(1, min(cdiv(target, C8 * n * strips), cdiv(hi, 4)));
  const int rpc = cdiv(hi, chunks);
  dim3 g(cdiv(hi, rpc) * strips, C8, n);
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, dim3(SW), 0, s, *gs, C8, hi, wi, idx_y, wgt_y, tys, tyj, txs, txj, txw, (T*)dx, rpc, cw, strips); };
    if (max_taps_x <= 8) { if (SW == 128) launch(k_bicubic_bwd_walk<T, 8, 128>); else if (SW == 256) launch(k_bicubic_bwd_walk<T, 8, 256>); else launch(k_bicubic_bwd_walk<T, 8, 512>); }
    else { if (SW == 128) launch(k_bicubic_bwd_walk<T, 12, 128>); else if (SW == 256) launch(k_bicubic_bwd_walk<T, 12, 256>); else launch(k_bicubic_bwd_walk<T, 12, 512>); }
  });
}

int mc_bicubic_bwd(const mc_grad_src* gs, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                   const int32_t* tys, const int32_t* tyj, const float* tyw, const int32_t* txs, const int32_t* txj,
                   const float* txw, int32_t dtype, void* dx, void* stream) {
  return mc_bicubic_bwd_taps(gs, n, c, hi, wi, ho, wo, tys, tyj, tyw, txs, txj, txw, 0, 0, dtype, dx, stream);
}

int mc_bicubic_bwd_separable(const mc_grad_src* gs, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                             const int32_t* tys, const int32_t* tyj, const float* tyw, const int32_t* txs, const int32_t* txj,
                             const float* txw, int32_t dtype, float* ws, void* dx, void* stream) {
  if (!gs || !dx || !ws || !tys || !tyj || !tyw || !txs || !txj || !txw || n <= 0 || c <= 0) return MC_EINVAL;
  int rc = check_gsrc(gs);
  if (rc) return rc;
  if (gs->hs != ho || gs->ws != wo || gs->kind == MC_GSRC_NONE) return MC_EINVAL;
  const int C8 = (c + 7) / 8;
  hipStream_t s = (hipStream_t)stream;
  dim3 g1(max(1, min(cdiv(hi * wo, 256), 2048)), C8, n), g2(max(1, min(cdiv(hi * wi, 256), 2048)), C8, n);
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_bicubic_bwd_ypass<T>, g1, dim3(256), 0, s, *gs, C8, hi, wo, tys, tyj, tyw, ws);
    hipLaunchKernelGGL(k_bicubic_bwd_xpass<T>, g2, dim3(256), 0, s, ws, C8, hi, wi, wo, txs, txj, txw, (T*)dx);
  });
}

}  // extern "C"

// Advection loss (DESIGN.md §9 "Advection loss", the reference's `-ad 1`): the temperature term of the FluidNet-family
// loss.  The predicted and the true velocity of an item are pushed through ONE explicit upwind advection step (ADNet.forward,
// k_adnet_step of loss.hip) on the item's own temperature x[6] and grid (4 x[0], 4 x[1], wall coordinates substituted); the
// Laplacian and the source cancel in the difference, so
//   e = dt_b (A(s u_p, s v_p) - A(s u_t, s v_t)),   A(u, v) = -u Dx(u) - v Dy(v)      on the interior,
//   loss_T = sum |e| (1 + [j == 1] + [j == W - 2]) / (N H W)        (the replicate-padded side columns; wall rows are 0),
// with the per-item CFL step dt_b of the TRUE velocity (no gradient through it).  The adjoint is pointwise in u_p, v_p (the
// stencil sits on T): one streaming kernel that read-modify-writes the interior of the gradient planes k_loss has written.
// The library is built with -ffp-contract=off: dt_b restates k_rollout_dxmin / k_rollout_reduce / k_rollout_dt expression for
// expression and is bit-identical to them on a shared grid.
#include "common.h"

namespace {

__device__ __forceinline__ float al_sgn(float x) { return (float)((x > 0.f) - (x < 0.f)); }

// X = 4 x[0], Y = 4 x[1] (exact in binary floating point) with the wall coordinates of ro_x / ro_y
__device__ __forceinline__ float al_x(const float* xs, int i, int j, int W) { return j == 0 ? 0.f : (j == W - 1 ? 4.f : 4.f * xs[(size_t)i * W + j]); }
__device__ __forceinline__ float al_y(const float* ys, int i, int j, int H, int W) { return i == 0 ? 0.f : (i == H - 1 ? 1.f : 4.f * ys[(size_t)i * W + j]); }

// Partial maxima / minima of the time step: ws [n][ADV_RB][2] = bits of max(|s u_t|, |s v_t|) and of min dx_l over the rows a
// block walks (uint order == float order for non-negative floats).  Every slot is written by its block, so nothing is reset
// and no two blocks touch one address: at 16 items a per-wave atomic form spent 65 us queueing on two cache lines.
constexpr int ADV_RB = MC_ADVECT_WS_PER_ITEM / 2;

__global__ __launch_bounds__(256) void k_advect_reduce(int H, int W, int ct, int xch, const float* __restrict__ uvp,
                                                       const float* __restrict__ x, const float* __restrict__ vs,
                                                       uint32_t* __restrict__ ws) {
  __shared__ float smx[4], smn[4];
  const int n = blockIdx.y;
  const size_t HW = (size_t)H * W;
  const float s = vs[n];
  const float* u = uvp + (size_t)n * ct * HW;
  const float* v = u + HW;
  const float* xs = x + (size_t)n * xch * HW;
  float mx = 0.f, mn = 3.4e38f;
  for (int i = 1 + blockIdx.x; i <= H - 2; i += gridDim.x)                     // rows: coalesced along W, no division
    for (int j = 1 + threadIdx.x; j <= W - 2; j += blockDim.x) {
      const size_t c = (size_t)i * W + j;
      mx = fmaxf(mx, fmaxf(fabsf(s * u[c]), fabsf(s * v[c])));
      mn = fminf(mn, al_x(xs, i, j, W) - al_x(xs, i, j - 1, W));
    }
  for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); mn = fminf(mn, __shfl_xor(mn, o, 64)); }
  if ((threadIdx.x & 63) == 0) { smx[threadIdx.x >> 6] = mx; smn[threadIdx.x >> 6] = mn; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t* w = ws + ((size_t)n * ADV_RB + blockIdx.x) * 2;
    w[0] = __float_as_uint(fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3])));
    w[1] = __float_as_uint(fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3])));
  }
}

// one wave per item: lane l takes partial l of the `blocks` written ones (max and min do not depend on the order)
__global__ __launch_bounds__(64) void k_advect_dt(int blocks, float cn, const uint32_t* __restrict__ ws, float* __restrict__ dt) {
  const int b = blockIdx.x, l = threadIdx.x;
  float uv = 0.f, dx = 3.4e38f;
  if (l < blocks) {
    uv = __uint_as_float(ws[((size_t)b * ADV_RB + l) * 2]);
    dx = __uint_as_float(ws[((size_t)b * ADV_RB + l) * 2 + 1]);
  }
  for (int o = 32; o > 0; o >>= 1) { uv = fmaxf(uv, __shfl_xor(uv, o, 64)); dx = fminf(dx, __shfl_xor(dx, o, 64)); }
  if (l != 0) return;
  const float dx2 = dx * dx;
  dt[b] = fminf(0.5f * cn * dx / uv, 0.5f * (dx2 * dx2) / (dx2 + dx2));                  // (uv == 0: +inf -> the diffusive limit)
}

// tile: 8 rows x 64 pixels per workgroup pass (a wave takes rows w and w + 4) with a one-pixel halo: T, X and Y of the tile
// live in LDS (7.9 KB).  Short tiles keep 4 workgroups a CU busy at 16 x 128 x 506; a 32-row tile left 2 and ran at 1.9 TB/s.
constexpr int AL_TH = 8, AL_TW = 64, AL_R = AL_TH / 4;
constexpr int AL_LW = AL_TW + 2, AL_LH = AL_TH + 2;

struct AdvGeom {
  int N, H, W, ct, xch, l2;
  float k;            // terms in the average: u, v[, p] and T
  int64_t pbs;        // batch stride of the prediction and gradient planes
};

__global__ __launch_bounds__(256) void k_advect_loss(AdvGeom g, const float* __restrict__ u_, const float* __restrict__ v_,
                                                     const float* __restrict__ uvp, const float* __restrict__ x_,
                                                     const float* __restrict__ vs, const float* __restrict__ dtp,
                                                     double* __restrict__ sums, float* __restrict__ gu_,
                                                     float* __restrict__ gv_, int tiles_x, int tiles) {
  const int H = g.H, W = g.W, n = blockIdx.y;
  const size_t HW = (size_t)H * W;
  const float* up = u_ + (size_t)n * g.pbs;
  const float* vp = v_ + (size_t)n * g.pbs;
  const float* ut = uvp + (size_t)n * g.ct * HW;
  const float* vt = ut + HW;
  const float* xs = x_ + (size_t)n * g.xch * HW;
  const float* ys = xs + HW;
  const float* T = xs + 6 * HW;
  float* gu = gu_ + (size_t)n * g.pbs;
  float* gv = gv_ + (size_t)n * g.pbs;
  const float s = vs[n], dt = dtp[n];
  const float cg = dt * s / (g.k * ((float)g.N * (float)HW));
  float a_t = 0.f;              // per-thread partial in f32 (<= a few dozen pixels), combined in f64 as k_loss does

  __shared__ float Ts[AL_LH * AL_LW], Xs[AL_LH * AL_LW], Ys[AL_LH * AL_LW];
  const int wv = threadIdx.x >> 6, lx = threadIdx.x & 63;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int y0 = (tile / tiles_x) * AL_TH, x0 = (tile % tiles_x) * AL_TW;
    // this thread's pixels first: their loads are in flight while the tile is staged
    float uu[AL_R], vv[AL_R], ur[AL_R], vr[AL_R], g0u[AL_R], g0v[AL_R];
    bool in[AL_R];
#pragma unroll
    for (int r = 0; r < AL_R; ++r) {
      const int y = y0 + wv + 4 * r, xx = x0 + lx;
      in[r] = y >= 1 && y <= H - 2 && xx >= 1 && xx <= W - 2;
      const size_t i = in[r] ? (size_t)y * W + xx : 0;
      uu[r] = in[r] ? up[i] : 0.f; vv[r] = in[r] ? vp[i] : 0.f;
      ur[r] = in[r] ? ut[i] : 0.f; vr[r] = in[r] ? vt[i] : 0.f;
      g0u[r] = in[r] ? gu[i] : 0.f; g0v[r] = in[r] ? gv[i] : 0.f;
    }
    __syncthreads();                                    // the previous tile has been consumed
    for (int t = threadIdx.x; t < AL_LH * AL_LW; t += 256) {
      const int ly = t / AL_LW, cx = t - ly * AL_LW, yy = y0 + ly - 1, xx = x0 + cx - 1;
      const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
      Ts[t] = ok ? T[(size_t)yy * W + xx] : 0.f;
      Xs[t] = ok ? al_x(xs, yy, xx, W) : 0.f;
      Ys[t] = ok ? al_y(ys, yy, xx, H, W) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < AL_R; ++r) {
      if (!in[r]) continue;
      const int ly = wv + 4 * r, y = y0 + ly, xx = x0 + lx;
      const size_t i = (size_t)y * W + xx;
      const int c = (ly + 1) * AL_LW + lx + 1;
      const float Tc = Ts[c];
      const float dxl = Xs[c] - Xs[c - 1], dxr = Xs[c + 1] - Xs[c];
      const float dyt = Ys[c] - Ys[c - AL_LW], dyb = Ys[c + AL_LW] - Ys[c];
      const float gl = (Tc - Ts[c - 1]) / dxl, gr = (Ts[c + 1] - Tc) / dxr;
      const float gt = (Tc - Ts[c - AL_LW]) / dyt, gb = (Ts[c + AL_LW] - Tc) / dyb;
      const float su = s * uu[r], sv = s * vv[r], tu = s * ur[r], tv = s * vr[r];
      const float DxP = (su > 0.f ? gl : 0.f) + (su < 0.f ? gr : 0.f);
      const float DyP = (sv > 0.f ? gt : 0.f) + (sv < 0.f ? gb : 0.f);
      const float DxT = (tu > 0.f ? gl : 0.f) + (tu < 0.f ? gr : 0.f);
      const float DyT = (tv > 0.f ? gt : 0.f) + (tv < 0.f ? gb : 0.f);
      const float e = dt * ((-su * DxP - sv * DyP) - (-tu * DxT - tv * DyT));
      const float w = 1.f + (xx == 1 ? 1.f : 0.f) + (xx == W - 2 ? 1.f : 0.f);        // the replicated side columns
      float de;                                                                        // d(term) / d(e)
      if (!g.l2) { a_t += fabsf(e) * w; de = al_sgn(e); }
      else { a_t += e * e * w; de = 2.f * e; }
      const float q = de * w * cg;
      gu[i] = g0u[r] + q * (-DxP);
      gv[i] = g0v[r] + q * (-DyP);
    }
  }
  __shared__ double red[4];
  const double rs = wave_sum_d((double)a_t);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = rs;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double r = red[0] + red[1] + red[2] + red[3];
    if (r != 0.0) atomicAdd(sums + MC_S_T_PLAIN, r);
  }
}

int al_check(int32_t n, int32_t h, int32_t w, int32_t x_channels) {
  if (n <= 0 || n > 65535 || h < 5 || w < 5 || x_channels < 7 || (int64_t)h * w > 0x7fffffffll) return MC_EINVAL;
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_advect_loss_dt(const float* uvp, int32_t uvp_channels, const float* x, int32_t x_channels, const float* scaler,
                      int32_t n, int32_t h, int32_t w, float cn_max, uint32_t* ws, float* dt, void* stream) {
  if (!uvp || !x || !scaler || !ws || !dt || uvp_channels < 2 || al_check(n, h, w, x_channels)) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = min(h - 2, ADV_RB);                                             // rows of the interior per block: >= 1
  hipLaunchKernelGGL(k_advect_reduce, dim3(blocks, n), dim3(256), 0, s, h, w, uvp_channels, x_channels, uvp, x, scaler, ws);
  hipLaunchKernelGGL(k_advect_dt, dim3(n), dim3(64), 0, s, blocks, cn_max, ws, dt);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_advect_loss(const mc_loss_desc* d, const float* u, const float* v, int64_t pred_batch_stride, const float* uvp,
                   const float* x, int32_t x_channels, const float* scaler, const float* dt, double* sums, float* gu, float* gv,
                   void* stream) {
  if (!d || !u || !v || !uvp || !x || !scaler || !dt || !sums || !gu || !gv) return MC_EINVAL;
  if (al_check(d->n, d->h, d->w, x_channels) || d->t_grad != -2 || pred_batch_stride < (int64_t)d->h * d->w) return MC_EINVAL;
  AdvGeom g;
  g.N = d->n; g.H = d->h; g.W = d->w; g.ct = d->p_pred ? 3 : 2; g.xch = x_channels; g.l2 = d->l2;
  g.k = (d->p_pred ? 3.f : 2.f) + 1.f;
  g.pbs = pred_batch_stride;
  const int tiles_x = cdiv(d->w, AL_TW), tiles = tiles_x * cdiv(d->h, AL_TH);
  dim3 grid(max(1, min(cdiv(1024, d->n), tiles)), d->n);
  hipLaunchKernelGGL(k_advect_loss, grid, dim3(256), 0, (hipStream_t)stream, g, u, v, uvp, x, scaler, dt, sums, gu, gv, tiles_x,
                     tiles);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

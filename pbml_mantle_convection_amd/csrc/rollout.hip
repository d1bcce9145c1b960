// Ensemble rollout (DESIGN.md §8 "Ensemble rollout"): B simulations advance together, each with its own CFL time step, its
// own clock t[b] and its own stopping time t_end[b].  The kernels restate k_adnet_reduce / k_adnet_dt / k_adnet_step of
// loss.hip expression for expression (the library is built with -ffp-contract=off), so a member's dt and next T are
// bit-identical to mc_adnet_step on that member alone.  Streaming f32 stencils and reductions: row-major coalesced access,
// wave-64 shuffles, f64 accumulation in a fixed order, no float atomics.
#include "common.h"

namespace {

__device__ __forceinline__ float ro_x(const float* xc, int i, int j, int W) { return j == 0 ? 0.f : (j == W - 1 ? 4.f : xc[(size_t)i * W + j]); }
__device__ __forceinline__ float ro_y(const float* yc, int i, int j, int H, int W) { return i == 0 ? 0.f : (i == H - 1 ? 1.f : yc[(size_t)i * W + j]); }

// flags[b] of one step
enum { RO_FROZEN = 0, RO_STEP = 1, RO_LAND = 2 };

// min over the interior of x[i][j] - x[i][j-1] (the dx_l of k_adnet_reduce); one block, once per reset
__global__ __launch_bounds__(256) void k_rollout_dxmin(const float* __restrict__ xc, int H, int W, float* __restrict__ dx_min) {
  __shared__ float sm[4];
  float mn = 3.4e38f;
  for (int idx = threadIdx.x; idx < (H - 2) * (W - 2); idx += blockDim.x) {
    const int i = idx / (W - 2) + 1, j = idx % (W - 2) + 1;
    mn = fminf(mn, ro_x(xc, i, j, W) - ro_x(xc, i, j - 1, W));
  }
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) dx_min[0] = fminf(fminf(sm[0], sm[1]), fminf(sm[2], sm[3]));
}

__global__ void k_rollout_ws_init(int B, uint32_t* __restrict__ ws) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) ws[b] = 0u;
}

// ws[b] = bits of max(|s_b u|, |s_b v|) over member b's interior (uint order == float order for non-negative floats; max
// is order-independent, so the atomic keeps the result deterministic)
__global__ __launch_bounds__(256) void k_rollout_reduce(int H, int W, int64_t uvs, const float* __restrict__ u_,
                                                        const float* __restrict__ v_, const float* __restrict__ vs,
                                                        uint32_t* __restrict__ ws) {
  const int n = blockIdx.y;
  const float s = vs ? vs[n] : 1.f;
  const float* u = u_ + (size_t)n * uvs;
  const float* v = v_ + (size_t)n * uvs;
  float mx = 0.f;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < (H - 2) * (W - 2); idx += gridDim.x * blockDim.x) {
    const int i = idx / (W - 2) + 1, j = idx % (W - 2) + 1;
    mx = fmaxf(mx, fmaxf(fabsf(s * u[(size_t)i * W + j]), fabsf(s * v[(size_t)i * W + j])));
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(ws + n, __float_as_uint(mx));
}

// dt[b] (f64 holding an f32 value, or the f64 remainder t_end - t of a landing step) and flags[b]
__global__ void k_rollout_dt(int B, float cn, const uint32_t* __restrict__ ws, const float* __restrict__ dx_min,
                             const double* __restrict__ t, const double* __restrict__ t_end, double* __restrict__ dt,
                             int32_t* __restrict__ flags) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float uv = __uint_as_float(ws[b]), dx = dx_min[0];
  const float dx2 = dx * dx;
  const float d = fminf(0.5f * cn * dx / uv, 0.5f * (dx2 * dx2) / (dx2 + dx2));       // (uv == 0: +inf -> the diffusive limit)
  const double tb = t[b], te = t_end[b];
  double dd = 0.0;
  int32_t f = RO_FROZEN;
  if (tb < te) {
    dd = (double)d;
    f = RO_STEP;
    if (tb + dd >= te) { dd = te - tb; f = RO_LAND; }
  }
  dt[b] = dd;
  flags[b] = f;
}

#define RO_PART 8      // doubles per (member, block): sum T, sum |sv|^2, sum Nu_bot terms, sum Nu_top terms, min T, max T, 2 spare

// k_adnet_step with dt[b]; a frozen member's T is copied.  Every block also leaves the f64 partial sums of the diagnostics
// of the field it has just written (and of the velocity it has just used) in part[(b * gridDim.x + block) * RO_PART].
__global__ __launch_bounds__(256) void k_rollout_step(int H, int W, int64_t uvs, const float* __restrict__ u_,
                                                      const float* __restrict__ v_, const float* __restrict__ vs,
                                                      const float* __restrict__ T_, const float* __restrict__ rqs,
                                                      const float* __restrict__ xc, const float* __restrict__ yc,
                                                      const double* __restrict__ dtp, const int32_t* __restrict__ flags,
                                                      float* __restrict__ out_, double* __restrict__ part) {
  __shared__ double sm[4][6];
  const int n = blockIdx.y;
  const float s = vs ? vs[n] : 1.f, dt = (float)dtp[n];
  const bool active = flags[n] != RO_FROZEN;
  const float* u = u_ + (size_t)n * uvs;
  const float* v = v_ + (size_t)n * uvs;
  const float* T = T_ + (size_t)n * H * W;
  const float rqc = rqs[n];
  float* out = out_ + (size_t)n * H * W;
  double sT = 0.0, sV = 0.0, sB = 0.0, sP = 0.0;
  float mn = 3.4e38f, mx = -3.4e38f;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < H * W; idx += gridDim.x * blockDim.x) {
    const int i = idx / W, j = idx - i * W;
    float r;
    if (!active) r = T[idx];
    else if (i == 0) r = 1.0f;
    else if (i == H - 1) r = 0.0f;
    else {
      const int jj = min(max(j, 1), W - 2);                   // side columns replicate their neighbour
      const size_t c = (size_t)i * W + jj;
      const float Tc = T[c], uu = s * u[c], vv = s * v[c];
      const float xm = ro_x(xc, i, jj - 1, W), x0 = ro_x(xc, i, jj, W), xp = ro_x(xc, i, jj + 1, W);
      const float ym = ro_y(yc, i - 1, jj, H, W), y0 = ro_y(yc, i, jj, H, W), yp = ro_y(yc, i + 1, jj, H, W);
      const float dxl = x0 - xm, dxr = xp - x0, dyt = y0 - ym, dyb = yp - y0;
      const float gl = (Tc - T[c - 1]) / dxl, gr = (T[c + 1] - Tc) / dxr;
      const float gt = (Tc - T[c - W]) / dyt, gb = (T[c + W] - Tc) / dyb;
      const float dTdx = (uu > 0.f ? gl : 0.f) + (uu < 0.f ? gr : 0.f);
      const float dTdy = (vv > 0.f ? gt : 0.f) + (vv < 0.f ? gb : 0.f);
      const float lap = (gr - gl) / (0.5f * dxr + 0.5f * dxl) + (gb - gt) / (0.5f * dyb + 0.5f * dyt);
      r = Tc + dt * (-uu * dTdx - vv * dTdy + lap + rqc);
    }
    out[idx] = r;
    const float su = s * u[idx], sv = s * v[idx];
    sT += (double)r;
    sV += (double)su * (double)su + (double)sv * (double)sv;
    mn = fminf(mn, r);
    mx = fmaxf(mx, r);
    if (j >= 1 && j <= W - 2) {
      if (i == 1) sB += (double)(((active ? 1.0f : T[j]) - r) / (yc[(size_t)W + j] - 0.f));
      if (i == H - 2) sP += (double)((r - (active ? 0.0f : T[(size_t)(H - 1) * W + j])) / (1.f - yc[(size_t)(H - 2) * W + j]));
    }
  }
  sT = wave_sum_d(sT); sV = wave_sum_d(sV); sB = wave_sum_d(sB); sP = wave_sum_d(sP);
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[wv][0] = sT; sm[wv][1] = sV; sm[wv][2] = sB; sm[wv][3] = sP; sm[wv][4] = mn; sm[wv][5] = mx; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    double a = sm[0][k];
    for (int w = 1; w < 4; ++w) a = k == 4 ? fmin(a, sm[w][k]) : (k == 5 ? fmax(a, sm[w][k]) : a + sm[w][k]);
    part[((size_t)n * gridDim.x + blockIdx.x) * RO_PART + k] = a;
  }
}

// One block; wave w takes members w, w + 4, ...: lane l adds blocks l, l + 64, ... in order, then the xor tree -- an order
// that depends on (H, W) alone.  Writes row cursor[0] of hist (dropped when the cursor stands at n_steps), advances the
// clocks of the members that stepped, and the cursor.
__global__ __launch_bounds__(256) void k_rollout_finalize(int B, int H, int W, int nblk, const double* __restrict__ part,
                                                          const double* __restrict__ dt, const int32_t* __restrict__ flags,
                                                          const double* __restrict__ t_end, double* __restrict__ t,
                                                          int32_t* __restrict__ steps, int32_t* __restrict__ cursor,
                                                          double* __restrict__ hist, int n_steps) {
  const int row = cursor[0];
  const int lane = threadIdx.x & 63;
  for (int b = threadIdx.x >> 6; b < B; b += blockDim.x >> 6) {
    double a[4] = {0.0, 0.0, 0.0, 0.0}, mn = 3.4e38, mx = -3.4e38;
    for (int k = lane; k < nblk; k += 64) {
      const double* p = part + ((size_t)b * nblk + k) * RO_PART;
      a[0] += p[0]; a[1] += p[1]; a[2] += p[2]; a[3] += p[3];
      mn = fmin(mn, p[4]); mx = fmax(mx, p[5]);
    }
    for (int o = 32; o > 0; o >>= 1) {
      for (int q = 0; q < 4; ++q) a[q] += __shfl_xor(a[q], o, 64);
      mn = fmin(mn, __shfl_xor(mn, o, 64)); mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    if (lane == 0) {
      const int32_t f = flags[b];
      const double d = dt[b];
      double tb = t[b];
      if (f == RO_LAND) tb = t_end[b];
      else if (f == RO_STEP) tb += d;
      if (f != RO_FROZEN) { t[b] = tb; steps[b] += 1; }
      if (row >= 0 && row < n_steps) {
        double* h = hist + ((size_t)row * B + b) * 8;
        const double cells = (double)H * (double)W, cols = (double)(W - 2);
        h[0] = tb; h[1] = d; h[2] = a[0] / cells; h[3] = sqrt(a[1] / cells); h[4] = a[2] / cols; h[5] = a[3] / cols;
        h[6] = mn; h[7] = mx;
      }
    }
  }
  __syncthreads();                                        // every wave has read the cursor
  if (threadIdx.x == 0 && row >= 0 && row < n_steps) cursor[0] = row + 1;
}

__global__ void k_rollout_set_cursor(int32_t* cursor, int32_t row) { cursor[0] = row; }

int ro_check(int32_t b, int32_t h, int32_t w) {
  if (b <= 0 || b > 65535 || h < 5 || w < 5 || (int64_t)h * w > 0x7fffffffll) return MC_EINVAL;
  return MC_OK;
}
int ro_blocks(int h, int w) { return max(1, min(cdiv(h * w, 256), 128)); }

}  // namespace

extern "C" {

int32_t mc_rollout_blocks(int32_t h, int32_t w) {
  if (ro_check(1, h, w)) return MC_EINVAL;
  return ro_blocks(h, w);
}

int mc_rollout_dx_min(const float* xc, int32_t h, int32_t w, float* dx_min, void* stream) {
  if (!xc || !dx_min || ro_check(1, h, w)) return MC_EINVAL;
  hipLaunchKernelGGL(k_rollout_dxmin, dim3(1), dim3(256), 0, (hipStream_t)stream, xc, h, w, dx_min);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_rollout_dt(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* dx_min,
                  const double* t, const double* t_end, int32_t b, int32_t h, int32_t w, float cn_max, uint32_t* ws, double* dt,
                  int32_t* flags, void* stream) {
  if (!u || !v || !dx_min || !t || !t_end || !ws || !dt || !flags || ro_check(b, h, w)) return MC_EINVAL;
  if (uv_stride < (int64_t)h * w) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_rollout_ws_init, dim3(cdiv(b, 256)), dim3(256), 0, s, b, ws);
  hipLaunchKernelGGL(k_rollout_reduce, dim3(ro_blocks(h, w), b), dim3(256), 0, s, h, w, uv_stride, u, v, vel_scale, ws);
  hipLaunchKernelGGL(k_rollout_dt, dim3(cdiv(b, 256)), dim3(256), 0, s, b, cn_max, ws, dx_min, t, t_end, dt, flags);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_rollout_step(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* T_prev,
                    const float* raq_scalar, const float* xc, const float* yc, const double* dt, const int32_t* flags, int32_t b,
                    int32_t h, int32_t w, float* T_next, double* partials, void* stream) {
  if (!u || !v || !T_prev || !raq_scalar || !xc || !yc || !dt || !flags || !T_next || !partials || ro_check(b, h, w))
    return MC_EINVAL;
  if (uv_stride < (int64_t)h * w || T_prev == T_next) return MC_EINVAL;
  hipLaunchKernelGGL(k_rollout_step, dim3(ro_blocks(h, w), b), dim3(256), 0, (hipStream_t)stream, h, w, uv_stride, u, v, vel_scale,
                     T_prev, raq_scalar, xc, yc, dt, flags, T_next, partials);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_rollout_finalize(const double* partials, const double* dt, const int32_t* flags, const double* t_end, double* t,
                        int32_t* steps, int32_t* cursor, double* hist, int32_t n_steps, int32_t b, int32_t h, int32_t w,
                        void* stream) {
  if (!partials || !dt || !flags || !t_end || !t || !steps || !cursor || !hist || n_steps <= 0 || ro_check(b, h, w))
    return MC_EINVAL;
  hipLaunchKernelGGL(k_rollout_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, b, h, w, ro_blocks(h, w), partials, dt, flags,
                     t_end, t, steps, cursor, hist, n_steps);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_rollout_set_cursor(int32_t* cursor, int32_t row, int32_t n_steps, void* stream) {
  if (!cursor || n_steps <= 0 || row < 0 || row > n_steps) return MC_EINVAL;
  hipLaunchKernelGGL(k_rollout_set_cursor, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor, row);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

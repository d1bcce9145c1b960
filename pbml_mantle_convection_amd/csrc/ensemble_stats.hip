// Ensemble rollout statistics (DESIGN.md §9 "Ensemble rollout: depth profiles, their time averages, saves at fixed simulated times"): horizontally
// averaged profiles of the state a step starts from, their time-weighted sums per member, and snapshots taken when a
// member's own clock passes its next saving time.  Streaming work beside the kernels of rollout.hip inside the captured
// step: row-major coalesced dword loads, wave-64 shuffles, f64 accumulation in a fixed order, no float atomics.
#include "common.h"

namespace {

enum { ES_FROZEN = 0 };      // flags[b] of mc_rollout_dt: 0 frozen, 1 step, 2 landing step

// One wave per row (b, i): lane l adds columns l, l + 64, ... in ascending order, then the xor tree, then / W: a row's
// four means depend on its own W values alone.  The same wave adds w * mean to the member's time sums when the member's
// weight w of this step is positive; the wave of row 0 also advances the member's weight sum and count.
__global__ __launch_bounds__(256) void k_ensemble_profiles(int B, int H, int W, int64_t uvs, const float* __restrict__ u_,
                                                           const float* __restrict__ v_, const float* __restrict__ vs,
                                                           const float* __restrict__ T_, const double* __restrict__ dt,
                                                           const int32_t* __restrict__ flags, const double* __restrict__ t,
                                                           const double* __restrict__ tas, double* __restrict__ prof,
                                                           double* __restrict__ acc, double* __restrict__ wsum,
                                                           int32_t* __restrict__ nacc) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * H) return;                                  // (whole waves: the shuffles below stay among live lanes)
  const int b = row / H, i = row - b * H, lane = threadIdx.x & 63;
  const float s = vs ? vs[b] : 1.f;
  const float* u = u_ + (size_t)b * uvs + (size_t)i * W;
  const float* v = v_ + (size_t)b * uvs + (size_t)i * W;
  const float* T = T_ + ((size_t)b * H + i) * W;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = lane; j < W; j += 64) {
    const float Tc = T[j], su = s * u[j], sv = s * v[j];
    a[0] += (double)Tc;
    a[1] += (double)su * (double)su;
    a[2] += (double)sv * (double)sv;
    a[3] += (double)sv * (double)Tc;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = wave_sum_d(a[q]) / (double)W;
  double w = 0.0;
  if (flags[b] != ES_FROZEN) {
    const double t0 = t[b], d = dt[b], ta = tas[b];
    w = (ta <= t0) ? d : fmax(0.0, (t0 + d) - ta);          // left Riemann sum: the state holds for the step it takes
  }
  if (lane < 4) {
    const size_t o = ((size_t)b * 4 + lane) * H + i;
    const double p = lane == 0 ? a[0] : (lane == 1 ? a[1] : (lane == 2 ? a[2] : a[3]));
    if (prof) prof[o] = p;
    if (w > 0.0) acc[o] += w * p;
  }
  if (i == 0 && lane == 0 && w > 0.0) { wsum[b] += w; nacc[b] += 1; }
}

// The reference loop's `if t > save_t: save_t = t + save_every`, per member on the member's own clock
__global__ void k_ensemble_save_rule(int B, int capacity, const double* __restrict__ t, const int32_t* __restrict__ flags,
                                     const double* __restrict__ save_every, double* __restrict__ next_save,
                                     int32_t* __restrict__ count, int32_t* __restrict__ missed, int32_t* __restrict__ slot,
                                     double* __restrict__ snap_t) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int32_t sl = -1;
  const double tb = t[b], every = save_every[b];
  if (flags[b] != ES_FROZEN && every > 0.0 && tb > next_save[b]) {
    const int32_t c = count[b];
    if (c >= 0 && c < capacity) {
      sl = c;
      snap_t[(size_t)b * capacity + c] = tb;
      count[b] = c + 1;
    } else {
      missed[b] += 1;
    }
    next_save[b] = tb + every;
  }
  slot[b] = sl;
}

__global__ __launch_bounds__(256) void k_ensemble_save_copy(int HW, int capacity, const float* __restrict__ T_,
                                                            const int32_t* __restrict__ slot, float* __restrict__ snaps) {
  const int b = blockIdx.y;
  const int32_t sl = slot[b];
  if (sl < 0 || sl >= capacity) return;
  const float* T = T_ + (size_t)b * HW;
  float* out = snaps + ((size_t)b * capacity + sl) * HW;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < HW; idx += gridDim.x * blockDim.x) out[idx] = T[idx];
}

int es_check(int32_t b, int32_t h, int32_t w) {
  if (b <= 0 || b > 65535 || h < 5 || w < 5 || (int64_t)h * w > 0x7fffffffll || (int64_t)b * h > 0x7fffffffll) return MC_EINVAL;
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_ensemble_profiles(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* T,
                         const double* dt, const int32_t* flags, const double* t, const double* t_avg_start, int32_t b,
                         int32_t h, int32_t w, double* prof, double* acc, double* wsum, int32_t* nacc, void* stream) {
  if (!u || !v || !T || !dt || !flags || !t || !t_avg_start || !acc || !wsum || !nacc || es_check(b, h, w)) return MC_EINVAL;
  if (uv_stride < (int64_t)h * w) return MC_EINVAL;
  hipLaunchKernelGGL(k_ensemble_profiles, dim3(cdiv(b * h, 4)), dim3(256), 0, (hipStream_t)stream, b, h, w, uv_stride, u, v,
                     vel_scale, T, dt, flags, t, t_avg_start, prof, acc, wsum, nacc);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_ensemble_snapshot(const float* T_new, const double* t, const int32_t* flags, const double* save_every, double* next_save,
                         int32_t* count, int32_t* missed, int32_t* slot, int32_t capacity, int32_t b, int32_t h, int32_t w,
                         float* snaps, double* snap_t, void* stream) {
  if (!T_new || !t || !flags || !save_every || !next_save || !count || !missed || !slot || !snaps || !snap_t || es_check(b, h, w))
    return MC_EINVAL;
  if (capacity <= 0 || T_new == snaps) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ensemble_save_rule, dim3(cdiv(b, 256)), dim3(256), 0, s, b, capacity, t, flags, save_every, next_save, count,
                     missed, slot, snap_t);
  hipLaunchKernelGGL(k_ensemble_save_copy, dim3(mc_rollout_blocks(h, w), b), dim3(256), 0, s, h * w, capacity, T_new, slot, snaps);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

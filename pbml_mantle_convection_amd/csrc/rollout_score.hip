// Rollout scoring (DESIGN.md §9 "Rollout scoring"): inside the captured step of the ensemble rollout, between mc_rollout_step
// and mc_rollout_finalize, every member whose own f64 clock passes one of its simulation's snapshot times within this step
// scores its temperature -- interpolated linearly in time between the state before and after the step -- against that
// snapshot: MAE, largest error, centred Pearson correlation, MAE of the horizontally averaged profile and the two means.
// One workgroup per member; it reads three scalars and leaves when nothing is due.  Row-major coalesced dword loads,
// wave-64 shuffles, f64 throughout in a fixed order that depends on (h, w) alone, plain vector stores, no atomics.
#include "common.h"

namespace {

enum { RS_FROZEN = 0, RS_STEP = 1, RS_LAND = 2 };   // flags[m] of mc_rollout_dt
enum { RS_WAVES = 16, RS_CHUNK = 128, RS_COLS = 8 };

__device__ __forceinline__ double rs_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// Adds (mx: takes the maximum of) v[0..n) in ascending order.  Eight LDS reads are issued before their eight dependent
// additions, so the chain costs its additions, not one LDS round trip per term.
template <bool MAX>
__device__ __forceinline__ double rs_ordered(const double* v, int n, double run) {
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    double x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = v[i + q];
#pragma unroll
    for (int q = 0; q < 8; ++q) run = MAX ? fmax(run, x[q]) : run + x[q];
  }
  for (; i < n; ++i) run = MAX ? fmax(run, v[i]) : run + v[i];
  return run;
}

// A lane's columns of one row, four at a time: the twelve loads are issued before the first of them is used; the sums still
// take the columns in ascending order.  f(a, b) adds one cell to the lane's sums.
template <class F>
__device__ __forceinline__ void rs_walk_row(int W, int lane, double theta, const float* __restrict__ p,
                                            const float* __restrict__ n, const float* __restrict__ r, F f) {
  int j = lane;
  for (; j + 192 < W; j += 256) {
    float pv[4], nv[4], rv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { pv[q] = p[j + 64 * q]; nv[q] = n[j + 64 * q]; rv[q] = r[j + 64 * q]; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double a0 = (double)pv[q];
      f(a0 + theta * ((double)nv[q] - a0), (double)rv[q]);
    }
  }
  for (; j < W; j += 64) {
    const double a0 = (double)p[j];
    f(a0 + theta * ((double)n[j] - a0), (double)r[j]);
  }
}

// Scores row k of member m.  Pass 1: wave q takes rows q, q + 16, ...; lane l adds columns l, l + 64, ... in ascending order,
// then the xor tree, then / W (the order of k_ensemble_profiles); the row means go to prof and, RS_CHUNK rows at a time, to
// LDS, where three threads add them over i ascending.  Pass 2: the same order inside a row; the five row results of up to
// RS_CHUNK rows wait in LDS until one thread per quantity has added them to its running value, i ascending.
__device__ void rs_score_row(int H, int W, const float* __restrict__ Tp, const float* __restrict__ Tn,
                             const float* __restrict__ Tr, double tau, double theta, double* __restrict__ out8,
                             double* __restrict__ pA, double* __restrict__ pB, double (*s_row)[RS_CHUNK], double* s_bc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double run = 0.0;                                         // threads 0..2: sum A_i, sum B_i, sum |A_i - B_i|
  for (int base = 0; base < H; base += RS_CHUNK) {
    const int rows = min(RS_CHUNK, H - base);
    for (int ii = wave; ii < rows; ii += RS_WAVES) {
      const size_t o = (size_t)(base + ii) * W;
      double sa = 0.0, sb = 0.0;
      rs_walk_row(W, lane, theta, Tp + o, Tn + o, Tr + o, [&](double a, double b) { sa += a; sb += b; });
      sa = wave_sum_d(sa) / (double)W;
      sb = wave_sum_d(sb) / (double)W;
      if (lane == 0) {
        pA[base + ii] = sa; pB[base + ii] = sb;
        s_row[0][ii] = sa; s_row[1][ii] = sb; s_row[2][ii] = fabs(sa - sb);
      }
    }
    __syncthreads();
    if (threadIdx.x < 3) run = rs_ordered<false>(s_row[threadIdx.x], rows, run);
    __syncthreads();                                        // the next chunk overwrites s_row
  }
  if (threadIdx.x < 3) s_bc[threadIdx.x] = run / (double)H;
  __syncthreads();
  const double Abar = s_bc[0], Bbar = s_bc[1];
  run = 0.0;                                                // threads 0..4: sum|a-b|, max|a-b|, Saa, Sbb, Sab
  for (int base = 0; base < H; base += RS_CHUNK) {
    const int rows = min(RS_CHUNK, H - base);
    for (int ii = wave; ii < rows; ii += RS_WAVES) {
      const size_t o = (size_t)(base + ii) * W;
      double e1 = 0.0, mx = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
      rs_walk_row(W, lane, theta, Tp + o, Tn + o, Tr + o, [&](double a, double b) {
        const double d = fabs(a - b), da = a - Abar, db = b - Bbar;
        e1 += d; mx = fmax(mx, d);
        aa += da * da; bb += db * db; ab += da * db;
      });
      e1 = wave_sum_d(e1); mx = rs_wave_max(mx); aa = wave_sum_d(aa); bb = wave_sum_d(bb); ab = wave_sum_d(ab);
      if (lane == 0) { s_row[0][ii] = e1; s_row[1][ii] = mx; s_row[2][ii] = aa; s_row[3][ii] = bb; s_row[4][ii] = ab; }
    }
    __syncthreads();
    if (threadIdx.x == 1) run = rs_ordered<true>(s_row[1], rows, run);
    else if (threadIdx.x < 5) run = rs_ordered<false>(s_row[threadIdx.x], rows, run);
    __syncthreads();                                        // the next chunk overwrites s_row
  }
  if (threadIdx.x < 5) s_bc[3 + threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cells = (double)H * (double)W, den = s_bc[5] * s_bc[6];
    out8[0] = tau; out8[1] = theta; out8[2] = s_bc[3] / cells; out8[3] = s_bc[4];
    out8[4] = den == 0.0 ? __longlong_as_double(0x7ff8000000000000ll) : s_bc[7] / sqrt(den);
    out8[5] = s_bc[2]; out8[6] = Abar; out8[7] = Bbar;
  }
  __syncthreads();                                          // s_bc is reused by the next row
}

__global__ __launch_bounds__(64 * RS_WAVES) void k_rollout_score(int H, int W, int capacity, const float* __restrict__ Tp_,
                                                                 const float* __restrict__ Tn_, const double* __restrict__ t,
                                                                 const double* __restrict__ dt, const int32_t* __restrict__ flags,
                                                                 const double* __restrict__ t_end, const float* __restrict__ truth,
                                                                 const double* __restrict__ truth_t,
                                                                 const int32_t* __restrict__ n_truth, int32_t* next,
                                                                 int32_t* scored, int32_t* skipped, double* __restrict__ table,
                                                                 double* prof) {
  __shared__ double s_row[5][RS_CHUNK];
  __shared__ double s_bc[RS_COLS];
  const int m = blockIdx.x;
  const int32_t f = flags[m];
  if (f == RS_FROZEN) return;
  const double t0 = t[m];
  double t1 = t0;                                           // k_rollout_finalize's expression: bitwise the clock it will store
  if (f == RS_LAND) t1 = t_end[m];
  else if (f == RS_STEP) t1 += dt[m];
  const int n = min(max(n_truth[m], 0), capacity);
  int k = max(next[m], 0);
  const double* tt = truth_t + (size_t)m * capacity;
  if (k >= n || !(tt[k] <= t1)) return;                     // the common step: nothing is due
  __syncthreads();                                          // every wave has read next[m] before thread 0 stores it
  const size_t HW = (size_t)H * W;
  const float *Tp = Tp_ + (size_t)m * HW, *Tn = Tn_ + (size_t)m * HW;
  int ns = 0, nk = 0;
  for (; k < n; ++k) {
    const double tau = tt[k];
    if (!(tau <= t1)) break;
    if (tau < t0) { ++nk; continue; }                       // a time the clock had already passed: the row stays as it is
    const double theta = t1 > t0 ? (tau - t0) / (t1 - t0) : 0.0;
    const size_t row = (size_t)m * capacity + k;
    rs_score_row(H, W, Tp, Tn, truth + row * HW, tau, theta, table + row * 8, prof + row * 2 * H, prof + (row * 2 + 1) * H, s_row,
                 s_bc);
    ++ns;
  }
  if (threadIdx.x == 0) { next[m] = k; scored[m] += ns; skipped[m] += nk; }
}

}  // namespace

extern "C" {

int mc_score_rollout(const float* T_prev, const float* T_next, const double* t, const double* dt, const int32_t* flags,
                     const double* t_end, const float* truth, const double* truth_t, const int32_t* n_truth, int32_t capacity,
                     int32_t b, int32_t h, int32_t w, int32_t* next, int32_t* scored, int32_t* skipped, double* table, double* prof,
                     void* stream) {
  if (!T_prev || !T_next || !t || !dt || !flags || !t_end || !truth || !truth_t || !n_truth || !next || !scored || !skipped ||
      !table || !prof)
    return MC_EINVAL;
  if (b <= 0 || b > 65535 || h < 5 || w < 5 || (int64_t)h * w > 0x7fffffffll || capacity <= 0 || T_prev == T_next) return MC_EINVAL;
  hipLaunchKernelGGL(k_rollout_score, dim3(b), dim3(64 * RS_WAVES), 0, (hipStream_t)stream, h, w, capacity, T_prev, T_next, t, dt,
                     flags, t_end, truth, truth_t, n_truth, next, scored, skipped, table, prof);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

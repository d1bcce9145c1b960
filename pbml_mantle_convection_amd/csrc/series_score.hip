// Series scoring (DESIGN.md §9 "Series scoring"): a trained Stokes net against the snapshots of a simulation, in the scaled
// space the network is trained in.  A store of N snapshots (T, u, v [N][h][w] f32, sim [N], prev [N]; paras, nd, inv_scale per
// simulation) stays in HBM; a work list idx[n_items] says what to score and a device cursor where the next batch of b slots
// starts.  Slot k holds item j = min(cursor + k, n_items - 1) and snapshot s = idx[j]; only slots with cursor + k < n_items
// write results, so ONE captured step of fixed batch b walks a list whose length is no multiple of b.
// Streaming work beside the network's forward: row-major coalesced dword loads, wave-64 shuffles, f64 accumulation in a
// fixed order, no float atomics.
#include "common.h"

namespace {

enum { SS_COLS = 10 };       // per row: sum|ut-uh|, sum|vt-vh|, sum|ut-ub|, sum|vt-vb|, max|ut|, max|vt|, max|ut-uh|, max|vt-vh|,
                             // sum|div(uh,vh)|, sum|div(ut,vt)|

struct SeriesList { const int32_t* idx; const int32_t* cursor; int32_t n_items, n_snap, n_sims; };

// item and snapshot of slot k; false: the slot lies past the end of the list (it still names a valid snapshot to gather)
__device__ __forceinline__ bool ss_slot(const SeriesList& q, int k, int& j, int& s) {
  const int c = q.cursor[0];
  const int64_t jj = (int64_t)max(c, 0) + k;
  j = (int)(jj < q.n_items ? jj : q.n_items - 1);
  s = min(max(q.idx[j], 0), q.n_snap - 1);                   // (a bad index never leaves the store)
  return c >= 0 && jj < q.n_items;
}
__device__ __forceinline__ int ss_sim(const int32_t* sim, int s, int n_sims) { return min(max(sim[s], 0), n_sims - 1); }

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// k_ts_build_input (loss.hip) expression for expression on T[idx[j]] with the parameters of that snapshot's simulation
__global__ __launch_bounds__(256) void k_series_build_input(SeriesList q, const float* __restrict__ T, int64_t ss,
                                                            const int32_t* __restrict__ sim, const float* __restrict__ xc,
                                                            const float* __restrict__ yc, const float* __restrict__ ycc,
                                                            const float* __restrict__ paras, const float* __restrict__ nd, int HW,
                                                            float* __restrict__ out) {
  const int n = blockIdx.y;
  int j, s;
  ss_slot(q, n, j, s);
  const int m = ss_sim(sim, s, q.n_sims);
  const float lnfkt = logf(paras[m * 3 + 1]), lnfkp = logf(paras[m * 3 + 2]);
  const float n0 = nd[m * 3], n1 = nd[m * 3 + 1], n2 = nd[m * 3 + 2];
  const float* Tn = T + (size_t)s * ss;
  float* o = out + (size_t)n * 7 * HW;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
    const float t = Tn[i];
    const float eta = fminf(fmaxf(expf(-lnfkt * t + lnfkp * (1.0f - ycc[i])), 1e-8f), 1.0f);
    o[i] = xc[i] * 0.25f;
    o[HW + i] = yc[i] * 0.25f;
    o[2 * (size_t)HW + i] = log10f(eta) * 0.125f;
    o[3 * (size_t)HW + i] = n0;
    o[4 * (size_t)HW + i] = n1;
    o[5 * (size_t)HW + i] = n2;
    o[6 * (size_t)HW + i] = t;
  }
}

// One wave per row (k, i): lane l takes columns l, l + 64, ... in ascending order, then the xor tree.  rows [b][10][H].
__global__ __launch_bounds__(256) void k_series_rows(SeriesList q, int B, int H, int W, int64_t uvs, const float* __restrict__ uh_,
                                                     const float* __restrict__ vh_, int64_t ss, const float* __restrict__ u_,
                                                     const float* __restrict__ v_, const int32_t* __restrict__ sim,
                                                     const int32_t* __restrict__ prev, const float* __restrict__ inv_scale,
                                                     double* __restrict__ rows) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * H) return;                                  // (whole waves: the shuffles below stay among live lanes)
  const int k = row / H, i = row - k * H, lane = threadIdx.x & 63;
  int j, s;
  if (!ss_slot(q, k, j, s)) return;
  const float is = inv_scale[ss_sim(sim, s, q.n_sims)];
  const int sp = prev[s];
  const bool has_prev = sp >= 0 && sp < q.n_snap;
  const bool inner = i >= 1 && i <= H - 2;
  const float* uh = uh_ + (size_t)k * uvs + (size_t)i * W;
  const float* vh = vh_ + (size_t)k * uvs + (size_t)i * W;
  const float* u = u_ + (size_t)s * ss + (size_t)i * W;
  const float* v = v_ + (size_t)s * ss + (size_t)i * W;
  const float* ub = u_ + (size_t)(has_prev ? sp : s) * ss + (size_t)i * W;
  const float* vb = v_ + (size_t)(has_prev ? sp : s) * ss + (size_t)i * W;
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, mx[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = lane; c < W; c += 64) {
    const float utf = u[c] * is, vtf = v[c] * is;
    const double ut = (double)utf, vt = (double)vtf;
    const double eu = fabs(ut - (double)uh[c]), ev = fabs(vt - (double)vh[c]);
    a[0] += eu;
    a[1] += ev;
    if (has_prev) {
      const float ubf = ub[c] * is, vbf = vb[c] * is;
      a[2] += fabs(ut - (double)ubf);
      a[3] += fabs(vt - (double)vbf);
    }
    mx[0] = fmax(mx[0], fabs(ut));
    mx[1] = fmax(mx[1], fabs(vt));
    mx[2] = fmax(mx[2], eu);
    mx[3] = fmax(mx[3], ev);
    if (inner && c >= 1 && c <= W - 2) {                     // get_mass(..., bc=False): central differences, unit spacing
      const double dp = 0.5 * ((double)uh[c + 1] - (double)uh[c - 1]) + 0.5 * ((double)vh[c + W] - (double)vh[c - W]);
      const float ue = u[c + 1] * is, uw = u[c - 1] * is, vn = v[c + W] * is, vs = v[c - W] * is;
      const double dt = 0.5 * ((double)ue - (double)uw) + 0.5 * ((double)vn - (double)vs);
      a[4] += fabs(dp);
      a[5] += fabs(dt);
    }
  }
#pragma unroll
  for (int n = 0; n < 6; ++n) a[n] = wave_sum_d(a[n]);
#pragma unroll
  for (int n = 0; n < 4; ++n) mx[n] = wave_max_d(mx[n]);
  if (lane == 0) {
    double* r = rows + (size_t)k * SS_COLS * H + i;
    const double qnan = __builtin_nan("");
    r[0] = a[0]; r[(size_t)H] = a[1];
    r[2 * (size_t)H] = has_prev ? a[2] : qnan; r[3 * (size_t)H] = has_prev ? a[3] : qnan;
    r[4 * (size_t)H] = mx[0]; r[5 * (size_t)H] = mx[1]; r[6 * (size_t)H] = mx[2]; r[7 * (size_t)H] = mx[3];
    r[8 * (size_t)H] = a[4]; r[9 * (size_t)H] = a[5];
  }
}

// One wave per slot.  The slot's rows pass through LDS 64 at a time (coalesced loads, one latency per chunk instead of one
// per row); lane n < 10 then walks column n over i ascending (sums added, maxima taken), and the lanes write the two error
// profiles from the values they staged.
enum { SS_CHUNK = 64 };
__global__ __launch_bounds__(64) void k_series_finalize(SeriesList q, int H, int W, const double* __restrict__ rows,
                                                        double* __restrict__ table, double* __restrict__ profile) {
  __shared__ double sm[SS_COLS][SS_CHUNK + 1];               // (+1: the ten columns start in different banks)
  const int k = blockIdx.x, lane = threadIdx.x;
  int j, s;
  if (!ss_slot(q, k, j, s)) return;                          // (the whole block: no barrier is left waiting)
  const double* r = rows + (size_t)k * SS_COLS * H;
  const bool is_max = lane >= 4 && lane <= 7;
  double acc = 0.0;
  for (int i0 = 0; i0 < H; i0 += SS_CHUNK) {
    const int n = min((int)SS_CHUNK, H - i0);
    if (lane < n) {
#pragma unroll
      for (int c = 0; c < SS_COLS; ++c) sm[c][lane] = r[(size_t)c * H + i0 + lane];
      profile[((size_t)j * 2) * H + i0 + lane] = sm[0][lane] / (double)W;
      profile[((size_t)j * 2 + 1) * H + i0 + lane] = sm[1][lane] / (double)W;
    }
    __syncthreads();
    if (lane < SS_COLS)
      for (int t = 0; t < n; ++t) acc = is_max ? fmax(acc, sm[lane][t]) : acc + sm[lane][t];
    __syncthreads();
  }
  if (lane < SS_COLS) {
    if (lane < 4) acc = acc / ((double)H * (double)W);
    if (lane >= 8) acc = acc / ((double)(H - 2) * (double)(W - 2));
    table[(size_t)j * SS_COLS + lane] = acc;
  }
}

// after every slot of the step has read the cursor (the launch before this one on the stream)
__global__ void k_series_advance(int32_t* cursor, int32_t b, int32_t n_items) {
  const int c = cursor[0];
  if (c >= 0 && c < n_items) cursor[0] = (int32_t)min((int64_t)c + b, (int64_t)n_items);
}

__global__ void k_series_set_cursor(int32_t* cursor, int32_t row) { cursor[0] = row; }

int ss_check(int32_t b, int32_t h, int32_t w, int32_t n_items, int32_t n_snap, int32_t n_sims) {
  if (b <= 0 || b > 65535 || h < 3 || w < 3 || n_items <= 0 || n_snap <= 0 || n_sims <= 0) return MC_EINVAL;
  if ((int64_t)h * w > 0x7fffffffll || (int64_t)b * h > 0x7fffffffll) return MC_EINVAL;
  return MC_OK;
}

}  // namespace

extern "C" {

int mc_series_build_input(const float* T, int64_t store_stride, const int32_t* sim, const float* xc, const float* yc,
                          const float* ycc, const float* paras, const float* paras_nd, const int32_t* idx, const int32_t* cursor,
                          int32_t n_items, int32_t n_snap, int32_t n_sims, int32_t b, int32_t h, int32_t w, float* out,
                          void* stream) {
  if (!T || !sim || !xc || !yc || !ycc || !paras || !paras_nd || !idx || !cursor || !out || ss_check(b, h, w, n_items, n_snap, n_sims))
    return MC_EINVAL;
  if (store_stride < (int64_t)h * w) return MC_EINVAL;
  const SeriesList q = {idx, cursor, n_items, n_snap, n_sims};
  dim3 grid(max(1, min(cdiv(h * w, 256), 1024)), b);
  hipLaunchKernelGGL(k_series_build_input, grid, dim3(256), 0, (hipStream_t)stream, q, T, store_stride, sim, xc, yc, ycc, paras,
                     paras_nd, h * w, out);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_series_score(const float* u_hat, const float* v_hat, int64_t uv_stride, const float* u, const float* v, int64_t store_stride,
                    const int32_t* sim, const int32_t* prev, const float* inv_scale, const int32_t* idx, const int32_t* cursor,
                    int32_t n_items, int32_t n_snap, int32_t n_sims, int32_t b, int32_t h, int32_t w, double* rows, void* stream) {
  if (!u_hat || !v_hat || !u || !v || !sim || !prev || !inv_scale || !idx || !cursor || !rows ||
      ss_check(b, h, w, n_items, n_snap, n_sims))
    return MC_EINVAL;
  if (uv_stride < (int64_t)h * w || store_stride < (int64_t)h * w) return MC_EINVAL;
  const SeriesList q = {idx, cursor, n_items, n_snap, n_sims};
  hipLaunchKernelGGL(k_series_rows, dim3(cdiv(b * h, 4)), dim3(256), 0, (hipStream_t)stream, q, b, h, w, uv_stride, u_hat, v_hat,
                     store_stride, u, v, sim, prev, inv_scale, rows);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_series_score_finalize(const double* rows, const int32_t* idx, int32_t* cursor, int32_t n_items, int32_t n_snap, int32_t b,
                             int32_t h, int32_t w, double* table, double* profile, void* stream) {
  if (!rows || !idx || !cursor || !table || !profile || ss_check(b, h, w, n_items, n_snap, 1)) return MC_EINVAL;
  const SeriesList q = {idx, cursor, n_items, n_snap, 1};
  hipLaunchKernelGGL(k_series_finalize, dim3(b), dim3(64), 0, (hipStream_t)stream, q, h, w, rows, table, profile);
  hipLaunchKernelGGL(k_series_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor, b, n_items);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_series_set_cursor(int32_t* cursor, int32_t row, int32_t n_items, void* stream) {
  if (!cursor || n_items <= 0 || row < 0 || row > n_items) return MC_EINVAL;
  hipLaunchKernelGGL(k_series_set_cursor, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor, row);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

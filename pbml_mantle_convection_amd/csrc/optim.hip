// Fused multi-tensor Adam over flat f32 buffers (torch.optim.Adam semantics: L2 weight decay folded
// into the gradient, bias-corrected moments; reference multigpu.py:761-763).
#include "common.h"

namespace {

__global__ void k_step_inc(int32_t* step) { if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1; }

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, int64_t numel, const float* __restrict__ lr_dev,
                                              float b1, float b2, float eps, float wd, float gscale,
                                              const int32_t* __restrict__ step_dev) {
  const float lr = *lr_dev;
  const int t = *step_dev;
  const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const int64_t n4 = numel / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gr = G[j] * gscale + wd * P[j];
      M[j] = b1 * M[j] + (1.f - b1) * gr;
      V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
      P[j] -= step_size * M[j] / (sqrtf(V[j]) * inv_sqrt_bc2 + eps);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < numel; i += stride) {
    float gr = g[i] * gscale + wd * p[i];
    float mi = b1 * m[i] + (1.f - b1) * gr, vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi; v[i] = vi;
    p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
  }
}

// ---- guarded step: ordered norm / non-finite reduction over the flat gradient, and an Adam launch that honours it ----
constexpr int GN_THREADS = 256;
constexpr int GN_MAX_BLOCKS = 1024;      // 4 blocks per CU; the single-block second launch takes four partials per lane

__host__ __device__ inline int grad_norm_blocks(int64_t numel) {
  int64_t b = (numel / 4 + GN_THREADS - 1) / GN_THREADS;
  return b > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : (b < 1 ? 1 : (int)b);
}

// Launch 1: per block one (sum of squares, non-finite count) pair, both f64, plain stores: ws[b] and ws[nblocks + b].  Every
// sum has a fixed order (lane -> wave butterfly -> waves in index order), so the pair is a function of the data alone.
__global__ __launch_bounds__(GN_THREADS) void k_grad_norm_partial(const float* __restrict__ g, int64_t numel,
                                                                  double* __restrict__ ws) {
  __shared__ double red[2][GN_THREADS / 64];
  const int64_t n4 = numel / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  uint32_t bad = 0;
  auto take = [&](const float4 gg) {
    s0 += (double)gg.x * (double)gg.x; s1 += (double)gg.y * (double)gg.y;
    s2 += (double)gg.z * (double)gg.z; s3 += (double)gg.w * (double)gg.w;
    bad += (uint32_t)!isfinite(gg.x) + (uint32_t)!isfinite(gg.y) + (uint32_t)!isfinite(gg.z) + (uint32_t)!isfinite(gg.w);
  };
  const float4* g4 = reinterpret_cast<const float4*>(g);
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {       // two loads in flight per lane
    const float4 a = g4[i], b = g4[i + stride];
    take(a);
    take(b);
  }
  if (i < n4) take(g4[i]);
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < numel; i += stride) {
    const float x = g[i];
    s0 += (double)x * (double)x;
    bad += (uint32_t)!isfinite(x);
  }
  const double sum = wave_sum_d((s0 + s1) + (s2 + s3)), cnt = wave_sum_d((double)bad);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = sum; red[1][wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0][0], c = red[1][0];
    for (int w = 1; w < GN_THREADS / 64; ++w) { a += red[0][w]; c += red[1][w]; }
    ws[blockIdx.x] = a;
    ws[gridDim.x + blockIdx.x] = c;
  }
}

// Launch 2 (one block): the partials summed as a fixed tree (lane t adds partials 4t .. 4t + 3 in index order, wave butterfly,
// the four waves in index order), the record, and the step counter (k_step_inc's job, taken only when the step is not skipped).
__global__ __launch_bounds__(GN_THREADS) void k_grad_guard_final(const double* __restrict__ ws, int nblocks, float gscale,
                                                                 float max_norm, int skip_nonfinite,
                                                                 mc_grad_guard* __restrict__ guard, int32_t* __restrict__ step) {
  static_assert(GN_MAX_BLOCKS <= 4 * GN_THREADS, "one pass of four partials per lane");
  __shared__ double red[2][GN_THREADS / 64];
  double a = 0.0, c = 0.0;
  for (int b = 4 * threadIdx.x; b < nblocks && b < 4 * (int)threadIdx.x + 4; ++b) { a += ws[b]; c += ws[nblocks + b]; }
  a = wave_sum_d(a);
  c = wave_sum_d(c);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = a; red[1][wave] = c; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = red[0][0], cnt = red[1][0];
  for (int w = 1; w < GN_THREADS / 64; ++w) { sum += red[0][w]; cnt += red[1][w]; }
  const double norm64 = (double)gscale * sqrt(sum);
  const uint32_t nonfinite = cnt >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)cnt;
  double coef = 1.0;
  if (max_norm > 0.f && nonfinite == 0) {
    coef = (double)max_norm / (norm64 + 1e-6);
    if (!(coef < 1.0)) coef = 1.0;
  }
  const uint32_t skip = (skip_nonfinite != 0 && nonfinite > 0) ? 1u : 0u;
  guard->norm = (float)norm64;
  guard->coef = (float)coef;
  guard->nonfinite = nonfinite;
  guard->skip = skip;
  if (skip) {
    guard->skipped += 1;
    guard->consecutive += 1;
  } else {
    guard->consecutive = 0;
    *step += 1;
  }
}

// k_adam with gs = gscale * guard->coef in place of gscale (formed once, in f32) and no store at all when guard->skip is set.
// A sibling, not a template flag on k_adam: the unguarded kernel stays the code it was.
__global__ __launch_bounds__(256) void k_adam_guarded(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, int64_t numel, const float* __restrict__ lr_dev,
                                                      float b1, float b2, float eps, float wd, float gscale,
                                                      const int32_t* __restrict__ step_dev,
                                                      const mc_grad_guard* __restrict__ guard) {
  if (guard->skip) return;
  const float gs = gscale * guard->coef;
  const float lr = *lr_dev;
  const int t = *step_dev;
  const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
  const float step_size = (float)((double)lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const int64_t n4 = numel / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gr = G[j] * gs + wd * P[j];
      M[j] = b1 * M[j] + (1.f - b1) * gr;
      V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
      P[j] -= step_size * M[j] / (sqrtf(V[j]) * inv_sqrt_bc2 + eps);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < numel; i += stride) {
    float gr = g[i] * gs + wd * p[i];
    float mi = b1 * m[i] + (1.f - b1) * gr, vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi; v[i] = vi;
    p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
  }
}

}  // namespace

extern "C" int mc_adam_step_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                 const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                 float grad_scale, int32_t* step_count_dev, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !lr_dev || !step_count_dev || numel <= 0) return MC_EINVAL;
  if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(64), 0, s, step_count_dev);
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq, numel, lr_dev, beta1,
                     beta2, eps, weight_decay, grad_scale, step_count_dev);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

extern "C" int mc_grad_norm_blocks(int64_t numel) { return numel <= 0 ? 0 : grad_norm_blocks(numel); }

extern "C" int mc_grad_guard_eval(const float* grad, int64_t numel, float grad_scale, float max_norm, int32_t skip_nonfinite,
                                  double* ws, mc_grad_guard* guard, int32_t* step_count_dev, void* stream) {
  if (!grad || !ws || !guard || !step_count_dev || numel <= 0) return MC_EINVAL;
  if (((uintptr_t)grad & 15) != 0 || ((uintptr_t)ws & 7) != 0 || ((uintptr_t)guard & 3) != 0) return MC_EINVAL;
  if (!(max_norm >= 0.f)) return MC_EINVAL;      // negative or NaN
  hipStream_t s = (hipStream_t)stream;
  const int blocks = grad_norm_blocks(numel);
  hipLaunchKernelGGL(k_grad_norm_partial, dim3((unsigned)blocks), dim3(GN_THREADS), 0, s, grad, numel, ws);
  hipLaunchKernelGGL(k_grad_guard_final, dim3(1), dim3(GN_THREADS), 0, s, ws, blocks, grad_scale, max_norm, (int)skip_nonfinite,
                     guard, step_count_dev);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

extern "C" int mc_adam_step_flat_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                                         const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                         float grad_scale, int32_t* step_count_dev, const mc_grad_guard* guard, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !lr_dev || !step_count_dev || !guard || numel <= 0) return MC_EINVAL;
  if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return MC_EINVAL;
  if (((uintptr_t)guard & 3) != 0) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_adam_guarded, dim3((unsigned)blocks), dim3(256), 0, s, param, grad, exp_avg, exp_avg_sq, numel, lr_dev,
                     beta1, beta2, eps, weight_decay, grad_scale, step_count_dev, guard);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

// GroupNorm + activation over the CB8 layout, forward and backward: statistics from the conv epilogue's partials, the
// fused normalise / activate / pool kernels and their one-launch forms for small layers, the three backward phases and the
// dz route, with the dropout variants and the host twins of the Philox generator (philox.h).
#include "common.h"
#include "philox.h"
#include "launch.h"
#include <type_traits>

namespace {

// =================================================================================================
// GroupNorm statistics from the conv epilogue's per-tile (sum, sumsq) partials
// =================================================================================================
// Per-channel totals of a [count][CP][2] partial array for the cpg channels of one group, one wave per (n, group).
// Lane l owns channel l % cpg and every (64 / cpg)-th partial; the lanes of a channel are then combined with a butterfly
// over the upper lane bits, so all channels of the group are summed at once (the former per-channel loop with two full
// double-precision wave reductions per channel made these tiny kernels ~15 us each, 50 launches per step).
// Requires cpg to be a power of two <= 64; afterwards EVERY lane holds the totals of its channel l % cpg.
__device__ __forceinline__ void group_channel_sums(const float* __restrict__ part, size_t base_n, int count, int CP, int c0,
                                                   int cpg, double& a1, double& a2) {
  const int lane = threadIdx.x & 63, cl = lane % cpg, per = 64 / cpg;
  a1 = 0.0; a2 = 0.0;
  int t = lane / cpg;
  // eight loads in flight (the loop was bound by one load latency per iteration: 30 us for the 1024 slots of a level-0 layer)
  for (; t + 7 * per < count; t += 8 * per) {
    float2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const float2*>(part + ((base_n + t + k * per) * CP + c0 + cl) * 2);
#pragma unroll
    for (int k = 0; k < 8; ++k) { a1 += (double)v[k].x; a2 += (double)v[k].y; }
  }
  for (; t < count; t += per) {
    const float2 v = *reinterpret_cast<const float2*>(part + ((base_n + t) * CP + c0 + cl) * 2);
    a1 += (double)v.x;
    a2 += (double)v.y;
  }
  for (int o = cpg; o < 64; o <<= 1) { a1 += __shfl_xor(a1, o, 64); a2 += __shfl_xor(a2, o, 64); }
}
__device__ __forceinline__ bool pow2_le64(int v) { return v >= 1 && v <= 64 && (v & (v - 1)) == 0; }

// (sum, sumsq) partials of a CB8 tensor: block (tile t, channel block cb, image n) sums the rows t, t + tiles, ...
template <typename T>
__global__ __launch_bounds__(256) void k_gn_partials(const T* __restrict__ y, int C8, int H, int W, int tiles,
                                                     float* __restrict__ part) {
  const int t = blockIdx.x, cb = blockIdx.y, n = blockIdx.z;
  float s[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) s[j] = 0.f;
  const int nrows = (H - t + tiles - 1) / tiles;
  for (int i = threadIdx.x; i < nrows * W; i += blockDim.x) {
    const int ry = i / W, xx = i - ry * W, yy = t + ry * tiles;
    float v[8];
    V8<T>::ld(y + cb8_index(n, cb, yy, xx, C8, H, W), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[2 * j] += v[j]; s[2 * j + 1] += v[j] * v[j]; }
  }
  __shared__ float red[4][16];
  int idx;
  float r = wave_sum16(s, threadIdx.x & 63, idx);
  if ((threadIdx.x & 3) == 0) red[threadIdx.x >> 6][idx] = r;
  __syncthreads();
  if (threadIdx.x < 16) {
    float tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    part[(((size_t)n * tiles + t) * (C8 * 8) + cb * 8 + (threadIdx.x >> 1)) * 2 + (threadIdx.x & 1)] = tot;
  }
}

// one wave per (n, g); also optional per-(n,c) means (block g handles its own channels) and the (scale, shift, mean,
// rstd) table [n][CP][4] read by consumers that normalise the raw conv output on load (same f32 expressions as gn_coef)
__global__ void k_gn_finalize(const float* __restrict__ part, int tiles, int C, int CP, int groups, int hw,
                              float eps, float* __restrict__ stats, float* __restrict__ chan_mean,
                              const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ coef4) {
  const int n = blockIdx.y, g = blockIdx.x;
  const int cpg = C / groups;
  double s = 0.0, ss = 0.0;
  const bool p2 = pow2_le64(cpg);
  if (p2) {
    double cs, css;
    group_channel_sums(part, (size_t)n * tiles, tiles, CP, g * cpg, cpg, cs, css);
    const int lane = threadIdx.x & 63;
    if (chan_mean && lane < cpg) chan_mean[n * C + g * cpg + lane] = (float)(cs / (double)hw);
    s = cs; ss = css;
    for (int o = 1; o < cpg; o <<= 1) { s += __shfl_xor(s, o, 64); ss += __shfl_xor(ss, o, 64); }
  } else {
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
      double cs = 0.0, css = 0.0;
      for (int t = threadIdx.x; t < tiles; t += blockDim.x) {
        const float* p = part + (((size_t)n * tiles + t) * CP + c) * 2;
        cs += (double)p[0];
        css += (double)p[1];
      }
      cs = wave_sum_d(cs);
      css = wave_sum_d(css);
      if (chan_mean && threadIdx.x == 0) chan_mean[n * C + c] = (float)(cs / (double)hw);
      s += cs;
      ss += css;
    }
  }
  // every lane holds the group totals
  const double m = (double)cpg * (double)hw;
  const double mean = s / m;
  double var = ss / m - mean * mean;
  if (var < 0.0) var = 0.0;
  const float meanf = (float)mean, rstdf = (float)(1.0 / sqrt(var + (double)eps));
  if (threadIdx.x == 0 && stats) {
    stats[((size_t)n * groups + g) * 2 + 0] = meanf;
    stats[((size_t)n * groups + g) * 2 + 1] = rstdf;
  }
  if (coef4) {
    for (int cl = threadIdx.x; cl < cpg; cl += blockDim.x) {
      const int c = g * cpg + cl;
      const float ga = gamma[c], be = beta[c];
      reinterpret_cast<float4*>(coef4)[(size_t)n * CP + c] = make_float4(rstdf * ga, be - meanf * rstdf * ga, meanf, rstdf);
    }
  }
}

// =================================================================================================
// a = act(GN(y)) [+ AvgPool(POOL)(a)]
// =================================================================================================
constexpr int GN_ROWS = 8;
// launch-shape knobs (environment overrides are for tuning runs only)
static int gn_fwd_vpt() { static int v = env_int("MC_GN_FWD_VPT", 8); return v; }
// rows per block of the backward-apply kernel (tools/bench_gn.py sweep on MI355X): 8 rows for wide images, more for narrow
// ones so that a block still streams >= 16 vectors per thread
// threads per block of the one-launch GroupNorm kernels (one block per (sample, channel block)): at 73-88 registers a
// 1024-thread block fills a CU alone, so a grid of more blocks than CUs (level 4: 16 channel blocks x 32 samples) ran in two
// rounds; 512-thread blocks sit two to a CU and finish in one (each thread then walks two pixels instead of one)
static int gn_small_threads(int blocks) {
  static int v = env_int("MC_GN_SMALL_THREADS", 0);
  if (v >= 512) return v;                       // (k_gn_act_small needs one wave per group of a channel block: >= 8 waves)
  return blocks > 256 ? 512 : 1024;             // in-step A/B, 1024 / auto / 512 / 256: 9.71 / 9.67 / 9.67 / 9.76 ms
}
static int gn_apply_rows(int h, int w) { static int v = env_int("MC_GN_ROWS", 0); if (v > 0) return v; return w > 256 ? GN_ROWS : (w > 32 ? 16 : 32); }

struct GnArgs {
  int N, C, C8, H, W, groups, cpg, post, act;
  const float* stats;
  const float* gamma;
  const float* beta;
};

__device__ __forceinline__ void gn_coef(const GnArgs& a, int n, int cb, float (&sc)[8], float (&sh)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int c = cb * 8 + j;
    if (a.post == MC_POST_GN_ACT && c < a.C) {
      int g = c / a.cpg;
      float mean = a.stats[((size_t)n * a.groups + g) * 2], rstd = a.stats[((size_t)n * a.groups + g) * 2 + 1];
      float ga = a.gamma[c], be = a.beta[c];
      sc[j] = rstd * ga;
      sh[j] = be - mean * rstd * ga;
    } else {
      sc[j] = (c < a.C) ? 1.f : 0.f;
      sh[j] = 0.f;
    }
  }
}

// Dropout after the activation (nn.Dropout at the end of a FluidLayer): a compile-time variant (DROP) of the kernels below.
// state = (seed_lo, seed_hi, step, 0) on the device; the mask of CB8 vector v is regenerated from it wherever it is needed
// (forward, both backward passes), never stored (csrc/philox.h).  scale = f32(65536 / keep16).
struct DropK { const uint32_t* state; uint32_t layer, keep16; float scale; };
struct DropSeed { uint32_t lo, hi, step; };
__device__ __forceinline__ DropSeed drop_seed(const DropK& d) { return DropSeed{d.state[0], d.state[1], d.state[2]}; }
__device__ __forceinline__ uint64_t drop_base(int n, int cb, int C8, int H, int W) {
  return ((uint64_t)n * C8 + cb) * (uint64_t)H * (uint64_t)W;
}
// ms[j] = kept ? scale : 0 for the 8 channels of vector v
__device__ __forceinline__ void drop_factors(const DropK& d, const DropSeed& sd, uint64_t v, float (&ms)[8]) {
  const uint32_t bits = mc_dropout_keep8(sd.lo, sd.hi, sd.step, d.layer, v, d.keep16);
#pragma unroll
  for (int j = 0; j < 8; ++j) ms[j] = ((bits >> j) & 1u) ? d.scale : 0.f;
}

template <typename T, int POOL, bool DROP = false>
__global__ void k_gn_act_fwd(GnArgs a, const T* __restrict__ y, T* __restrict__ out, T* __restrict__ pooled, DropK dk) {
  static_assert(!DROP || POOL == 1, "dropout layers are not pooled in the same launch");
  // one thread per POOLxPOOL pixel block of one channel block
  const int Hb = (a.H + POOL - 1) / POOL, Wb = (a.W + POOL - 1) / POOL;
  const int Hp = a.H / POOL, Wp = a.W / POOL;
  const int n = (int)blockIdx.z, cb = blockIdx.y;
  float sc[8], sh[8];
  gn_coef(a, n, cb, sc, sh);
  const int act = a.post == MC_POST_NONE ? MC_ACT_NONE : a.act;
  DropSeed sd = {0, 0, 0};
  uint64_t vbase = 0;
  if constexpr (DROP) { sd = drop_seed(dk); vbase = drop_base(n, cb, a.C8, a.H, a.W); }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hb * Wb; i += gridDim.x * blockDim.x) {
    int by = i / Wb, bx = i % Wb;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < POOL; ++dy)
#pragma unroll
      for (int dx = 0; dx < POOL; ++dx) {
        int yy = by * POOL + dy, xx = bx * POOL + dx;
        if (yy < a.H && xx < a.W) {
          float v[8];
          size_t idx = cb8_index(n, cb, yy, xx, a.C8, a.H, a.W);
          V8<T>::ld(y + idx, v);
          act_fwd8<FastMath<T>::value>(v, sc, sh, act, v);
          if constexpr (DROP) {
            float ms[8];
            drop_factors(dk, sd, vbase + (uint32_t)(yy * a.W + xx), ms);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] *= ms[j];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += v[j];
          if (out) V8<T>::st(out + idx, v);
        }
      }
    if (POOL > 1 && by < Hp && bx < Wp) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= 1.0f / (POOL * POOL);
      V8<T>::st(pooled + cb8_index(n, cb, by, bx, a.C8, Hp, Wp), acc);
    }
  }
}

// a = act(GN(y)) and AvgPool2d(2)(a) with COALESCED rows: a thread handles the pixels (2r, x) and (2r + 1, x), so consecutive
// lanes read and write consecutive 16-byte vectors, and takes the horizontal neighbour's sums from the adjacent lane (needs an
// even width; the one-thread-per-2x2-block form above touches every second vector of a row per instruction: 182 us instead
// of ~125 us at 506 x 512).  Pooling uses the f32 activation values, like the block form.
template <typename T>
__global__ void k_gn_act_fwd_pool2_rows(GnArgs a, const T* __restrict__ y, T* __restrict__ out, T* __restrict__ pooled) {
  const int n = (int)blockIdx.z, cb = blockIdx.y;
  float sc[8], sh[8];
  gn_coef(a, n, cb, sc, sh);
  const int act = a.post == MC_POST_NONE ? MC_ACT_NONE : a.act;
  const size_t base = ((size_t)n * a.C8 + cb) * a.H * a.W * 8;
  const int Hh = (a.H + 1) / 2, Hp = a.H / 2, Wp = a.W / 2;
  const int total = Hh * a.W, span = gridDim.x * blockDim.x;             // (span and W are even: lanes 2k, 2k + 1 share a row)
  for (int i0 = blockIdx.x * blockDim.x; i0 < total; i0 += span) {
    const int i = i0 + threadIdx.x;
    const bool live = i < total;
    const int r = live ? i / a.W : 0, x = live ? i - r * a.W : 0;
    float s8[8], v0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, v1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
      const size_t i0e = base + ((size_t)(2 * r) * a.W + x) * 8;
      V8<T>::ld(y + i0e, v0);
      act_fwd8<FastMath<T>::value>(v0, sc, sh, act, v0);
      if (out) V8<T>::st(out + i0e, v0);
      if (2 * r + 1 < a.H) {
        V8<T>::ld(y + i0e + (size_t)a.W * 8, v1);
        act_fwd8<FastMath<T>::value>(v1, sc, sh, act, v1);
        if (out) V8<T>::st(out + i0e + (size_t)a.W * 8, v1);
      }
    }
    // ((a00 + a01) + a10) + a11: the summation order of the block form, of k_gn_act_small and of k_avgpool (bit-identical
    // pooled tensors whichever kernel a layer takes)
#pragma unroll
    for (int j = 0; j < 8; ++j) s8[j] = 0.25f * (((v0[j] + __shfl_xor(v0[j], 1, 64)) + v1[j]) + __shfl_xor(v1[j], 1, 64));
    if (live && (x & 1) == 0 && r < Hp && (x >> 1) < Wp)
      V8<T>::st(pooled + (((size_t)n * a.C8 + cb) * Hp * Wp + (size_t)r * Wp + (x >> 1)) * 8, s8);
  }
}

// Small layers: GroupNorm statistics from the conv's partial sums AND a = act(GN(y)) [+ AvgPool] in one launch, one block per
// (sample, channel block); needs every group inside one channel block (channels per group 1, 2, 4 or 8).  The (mean, rstd)
// pairs are also written out for the backward pass.  Same f64 sums and f32 expressions as k_gn_finalize / gn_coef.
template <typename T, int POOL, bool DROP = false>
__global__ __launch_bounds__(1024) void k_gn_act_small(GnArgs a, const T* __restrict__ y, const float* __restrict__ part, int tiles,
                                                       float eps, float* __restrict__ stats_out, T* __restrict__ out,
                                                       T* __restrict__ pooled, DropK dk) {
  static_assert(!DROP || POOL == 1, "dropout layers are not pooled in the same launch");
  const int n = (int)blockIdx.y, cb = blockIdx.x, CP = a.C8 * 8;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float s_mean[8], s_rstd[8];
  const int ng = 8 / a.cpg;                                   // groups of this channel block (some may lie beyond C)
  if (wave < ng) {
    const int c0 = cb * 8 + wave * a.cpg;
    if (c0 < a.C) {
      double cs, css;
      group_channel_sums(part, (size_t)n * tiles, tiles, CP, c0, a.cpg, cs, css);
      for (int o = 1; o < a.cpg; o <<= 1) { cs += __shfl_xor(cs, o, 64); css += __shfl_xor(css, o, 64); }
      const double m = (double)a.cpg * (double)a.H * (double)a.W;
      const double mean = cs / m;
      double var = css / m - mean * mean;
      if (var < 0.0) var = 0.0;
      const float meanf = (float)mean, rstdf = (float)(1.0 / sqrt(var + (double)eps));
      if (lane == 0) {
        s_mean[wave] = meanf; s_rstd[wave] = rstdf;
        const int g = c0 / a.cpg;
        stats_out[((size_t)n * a.groups + g) * 2] = meanf;
        stats_out[((size_t)n * a.groups + g) * 2 + 1] = rstdf;
      }
    }
  }
  __syncthreads();
  float sc[8], sh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cb * 8 + j;
    sc[j] = 0.f; sh[j] = 0.f;
    if (c < a.C) {
      const float mean = s_mean[j / a.cpg], rstd = s_rstd[j / a.cpg], ga = a.gamma[c], be = a.beta[c];
      sc[j] = rstd * ga;
      sh[j] = be - mean * rstd * ga;
    }
  }
  const int Hb = (a.H + POOL - 1) / POOL, Wb = (a.W + POOL - 1) / POOL;
  const int Hp = a.H / POOL, Wp = a.W / POOL;
  DropSeed sd = {0, 0, 0};
  uint64_t vbase = 0;
  if constexpr (DROP) { sd = drop_seed(dk); vbase = drop_base(n, cb, a.C8, a.H, a.W); }
  for (int i = threadIdx.x; i < Hb * Wb; i += blockDim.x) {
    const int by = i / Wb, bx = i - by * Wb;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int dy = 0; dy < POOL; ++dy)
#pragma unroll
      for (int dx = 0; dx < POOL; ++dx) {
        const int yy = by * POOL + dy, xx = bx * POOL + dx;
        if (yy < a.H && xx < a.W) {
          float v[8];
          const size_t idx = cb8_index(n, cb, yy, xx, a.C8, a.H, a.W);
          V8<T>::ld(y + idx, v);
          act_fwd8<FastMath<T>::value>(v, sc, sh, a.act, v);
          if constexpr (DROP) {
            float ms[8];
            drop_factors(dk, sd, vbase + (uint32_t)(yy * a.W + xx), ms);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] *= ms[j];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += v[j];
          V8<T>::st(out + idx, v);
        }
      }
    if (POOL > 1 && by < Hp && bx < Wp) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] *= 1.0f / (POOL * POOL);
      V8<T>::st(pooled + cb8_index(n, cb, by, bx, a.C8, Hp, Wp), acc);
    }
  }
}

// =================================================================================================
// backward of act(GN(y))
// =================================================================================================
// phase 1: partial[n][blk][c][2] = (sum dz, sum dz * yhat) over this block's pixels
// GK: compile-time (source 0, source 1) kinds: 0 = decided at run time, 1 = (PADFOLD, NONE), 2 = (PLAIN, NONE),
// 3 = (PADFOLD, PADFOLD_POOL)
template <int GK> struct GKinds {
  static constexpr int k0 = GK == 1 ? MC_GSRC_PADFOLD : (GK == 2 ? MC_GSRC_PLAIN : (GK == 3 ? MC_GSRC_PADFOLD : -1));
  static constexpr int k1 = (GK == 1 || GK == 2) ? MC_GSRC_NONE : (GK == 3 ? MC_GSRC_PADFOLD_POOL : -1);
};
static int gkind_of(const mc_grad_src& g0, const mc_grad_src& g1) {
  if (g0.c8_total > 0 || g1.c8_total > 0) return 0;        // slices of a concatenated tensor: generic path
  if (g0.kind == MC_GSRC_PADFOLD && g1.kind == MC_GSRC_NONE) return 1;
  if (g0.kind == MC_GSRC_PLAIN && g1.kind == MC_GSRC_NONE) return 2;
  if (g0.kind == MC_GSRC_PADFOLD && g1.kind == MC_GSRC_PADFOLD_POOL) return 3;
  return 0;
}
// The variant of a GroupNorm-backward kernel one launch takes: (T, TY) from the dtype; f32 always decides its source kinds at
// run time (GK = 0), the 16-bit types take the compile-time kinds gk = gkind_of(s0, s1); dropout is GK = 0, DROP = true in every
// type (the Philox rounds, not the fetch, bound these variants).  f(TypeTag<T>, TypeTag<TY>, integral_constant<int, GK>,
// bool_constant<DROP>); MC_EUNSUPPORTED without a call for an unknown dtype.
template <typename F> static int with_gn_bwd_variant(int dtype, int gk, bool drop, F&& f) {
  return with_grad_y_types(dtype, [&](auto t, auto ty) {
    using GK0 = std::integral_constant<int, 0>;
    if (drop) f(t, ty, GK0{}, std::true_type{});
    else if constexpr (std::is_same<typename decltype(t)::type, float>::value) f(t, ty, GK0{}, std::false_type{});
    else switch (gk) {
      case 1: f(t, ty, std::integral_constant<int, 1>{}, std::false_type{}); break;
      case 2: f(t, ty, std::integral_constant<int, 2>{}, std::false_type{}); break;
      case 3: f(t, ty, std::integral_constant<int, 3>{}, std::false_type{}); break;
      default: f(t, ty, GK0{}, std::false_type{});
    }
  });
}

// TY: storage type of y (MC_MIX16: y is f16 while the gradient tensors T are bf16)
template <typename T, int GK, typename TY = T, bool DROP = false>
__global__ __launch_bounds__(256, DROP ? 5 : 6) void k_gn_bwd_reduce(GnArgs a, const TY* __restrict__ y, mc_grad_src g0,
                                                       mc_grad_src g1, float* __restrict__ part, int CP, DropK dk) {
  const int n = (int)blockIdx.z, cb = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  float sc[8], sh[8], mean[8], rstd[8];
  gn_coef(a, n, cb, sc, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int c = cb * 8 + j;
    if (c < a.C) {
      int g = c / a.cpg;
      mean[j] = a.stats[((size_t)n * a.groups + g) * 2];
      rstd[j] = a.stats[((size_t)n * a.groups + g) * 2 + 1];
    } else { mean[j] = 0.f; rstd[j] = 0.f; }
  }
  float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // rows blk, blk + nblk, ... of this block, flattened with the columns so that narrow images (W < 256) still use every
  // thread (a per-row loop left 7/8 of the threads idle at the deep levels: ~25 us floor per launch)
  const int nrows = (a.H - blk + nblk - 1) / nblk;
#ifndef MC_GN_RED_UNROLL
#define MC_GN_RED_UNROLL 1   /* A/B on MI355X: 2 = no gain (4.1 TB/s either way), 4 spills (3x slower) */
#endif
  // MC_GN_RED_UNROLL positions per iteration, every load issued before the first use: the loop is bound by the bytes it
  // keeps in flight (two 16-byte loads per position), not by arithmetic
  const int total = nrows * a.W;
  DropSeed sd = {0, 0, 0};
  uint64_t vbase = 0;
  if constexpr (DROP) { sd = drop_seed(dk); vbase = drop_base(n, cb, a.C8, a.H, a.W); }
  for (int i0 = threadIdx.x; i0 < total; i0 += blockDim.x * MC_GN_RED_UNROLL) {
    float v[MC_GN_RED_UNROLL][8], da[MC_GN_RED_UNROLL][8];
#pragma unroll
    for (int u = 0; u < MC_GN_RED_UNROLL; ++u) {
      const int i = min(i0 + u * (int)blockDim.x, total - 1);
      const int ry = i / a.W, xx = i - ry * a.W, yy = blk + ry * nblk;
#pragma unroll
      for (int j = 0; j < 8; ++j) da[u][j] = 0.f;
      V8<TY>::ld(y + cb8_index(n, cb, yy, xx, a.C8, a.H, a.W), v[u]);
      grad_fetch_add<T, GKinds<GK>::k0>(g0, n, cb, yy, xx, a.C8, da[u]);
      grad_fetch_add<T, GKinds<GK>::k1>(g1, n, cb, yy, xx, a.C8, da[u]);
      if constexpr (DROP) {
        float ms[8];
        drop_factors(dk, sd, vbase + (uint32_t)(yy * a.W + xx), ms);
#pragma unroll
        for (int j = 0; j < 8; ++j) da[u][j] *= ms[j];
      }
    }
#pragma unroll
    for (int u = 0; u < MC_GN_RED_UNROLL; ++u) {
      const float live = (i0 + u * (int)blockDim.x < total) ? 1.f : 0.f;     // the clamped tail position contributes nothing
      float ga[8];
      act_bwd8<FastMath<T>::value>(v[u], sc, sh, a.act, ga);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float dz = live * da[u][j] * ga[j];
        s1[j] += dz;
        s2[j] += dz * (v[u][j] - mean[j]) * rstd[j];
      }
    }
  }
  __shared__ float red[4][16];
  {
    float s[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) { s[2 * j] = s1[j]; s[2 * j + 1] = s2[j]; }
    int idx;
    float r = wave_sum16(s, threadIdx.x & 63, idx);
    if ((threadIdx.x & 3) == 0) red[threadIdx.x >> 6][idx] = r;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    float r = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    int c = cb * 8 + (threadIdx.x >> 1);
    part[(((size_t)n * nblk + blk) * CP + c) * 2 + (threadIdx.x & 1)] = r;
  }
}

// phase 2: one block per group g: m12[n][g] = (sum_c gamma_c s1, sum_c gamma_c s2) / M for every sample, and
// dgamma[c] += sum_n s2[n][c], dbeta[c] += sum_n s1[n][c].  DETERMINISTIC: the 16 waves of the block take the samples
// round-robin, park their per-(sample, channel) sums in LDS, and one thread per (channel, kind) adds them in sample order
// (round 1 used N float atomics per channel: the training step was not reproducible from run to run).
// One row of the table mc_conv2d_wgrad_dz reads: dzc[n][c] = (cA, cB, cC, mean) with dy = cA dz + (cB (z - mean) + cC), the
// expressions of k_gn_bwd_apply_dz on the same f32 (m1, m2) that go to m12.
__device__ __forceinline__ void write_dz_coef(const float* __restrict__ coef4, float* __restrict__ dzc, int n, int CP, int c,
                                              float m1, float m2) {
  const float4 c4 = reinterpret_cast<const float4*>(coef4)[(size_t)n * CP + c];
  reinterpret_cast<float4*>(dzc)[(size_t)n * CP + c] = make_float4(c4.x, -c4.w * c4.w * m2, -c4.w * m1, c4.z);
}

constexpr int GNF_CHUNK = 256;          // samples per LDS round
__global__ __launch_bounds__(1024) void k_gn_bwd_finalize(const float* __restrict__ part, int N, int blocks, int C, int CP,
                                                          int groups, int hw, const float* __restrict__ gamma,
                                                          float* __restrict__ m12, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, const float* __restrict__ coef4,
                                                          float* __restrict__ dzc) {
  const int g = blockIdx.x, cpg = C / groups;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  __shared__ float sm[GNF_CHUNK][16];                      // [sample][2 * channel-in-group + (0: s1, 1: s2)], cpg <= 8
  const double M = (double)cpg * (double)hw;
  if (pow2_le64(cpg) && cpg <= 8) {
    float tot = 0.f;                                        // thread t < 2 cpg: running sum of value t over the samples
    for (int n0 = 0; n0 < N; n0 += GNF_CHUNK) {
      const int nn = min(GNF_CHUNK, N - n0);
      for (int k = wave; k < nn; k += nwaves) {
        const int n = n0 + k;
        double a1, a2;
        group_channel_sums(part, (size_t)n * blocks, blocks, CP, g * cpg, cpg, a1, a2);
        const int c = g * cpg + (lane % cpg);
        if (lane < cpg) { sm[k][2 * lane] = (float)a1; sm[k][2 * lane + 1] = (float)a2; }
        const float ga = gamma ? gamma[c] : 1.f;
        double m1 = ga * a1, m2 = ga * a2;
        for (int o = 1; o < cpg; o <<= 1) { m1 += __shfl_xor(m1, o, 64); m2 += __shfl_xor(m2, o, 64); }
        if (lane == 0 && m12) {
          m12[((size_t)n * groups + g) * 2 + 0] = (float)(m1 / M);
          m12[((size_t)n * groups + g) * 2 + 1] = (float)(m2 / M);
        }
        if (dzc) {                                          // (lane 0's values: the ones m12 holds)
          const float f1 = __shfl((float)(m1 / M), 0, 64), f2 = __shfl((float)(m2 / M), 0, 64);
          if (lane < cpg) write_dz_coef(coef4, dzc, n, CP, c, f1, f2);
        }
      }
      __syncthreads();
      if ((int)threadIdx.x < 2 * cpg)
        for (int k = 0; k < nn; ++k) tot += sm[k][threadIdx.x];
      __syncthreads();
    }
    if ((int)threadIdx.x < 2 * cpg) {
      const int c = g * cpg + (threadIdx.x >> 1);
      if (threadIdx.x & 1) { if (dgamma) dgamma[c] += tot; }
      else if (dbeta) dbeta[c] += tot;
    }
    return;
  }
  // general group width: one wave walks the samples and the channels in order
  if (wave != 0) return;
  for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
    float tg = 0.f, tb = 0.f;
    for (int n = 0; n < N; ++n) {
      double a1 = 0.0, a2 = 0.0;
      for (int t = lane; t < blocks; t += 64) {
        const float* p = part + (((size_t)n * blocks + t) * CP + c) * 2;
        a1 += (double)p[0];
        a2 += (double)p[1];
      }
      a1 = wave_sum_d(a1);
      a2 = wave_sum_d(a2);
      tb += (float)a1;
      tg += (float)a2;
    }
    if (lane == 0) {
      if (dgamma) dgamma[c] += tg;
      if (dbeta) dbeta[c] += tb;
    }
  }
  if (m12) {
    for (int n = 0; n < N; ++n) {
      double m1 = 0.0, m2 = 0.0;
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        double a1 = 0.0, a2 = 0.0;
        for (int t = lane; t < blocks; t += 64) {
          const float* p = part + (((size_t)n * blocks + t) * CP + c) * 2;
          a1 += (double)p[0];
          a2 += (double)p[1];
        }
        a1 = wave_sum_d(a1);
        a2 = wave_sum_d(a2);
        const float ga = gamma ? gamma[c] : 1.f;
        m1 += ga * a1;
        m2 += ga * a2;
      }
      if (lane == 0) {
        m12[((size_t)n * groups + g) * 2 + 0] = (float)(m1 / M);
        m12[((size_t)n * groups + g) * 2 + 1] = (float)(m2 / M);
        if (dzc)
          for (int c = g * cpg; c < (g + 1) * cpg; ++c) write_dz_coef(coef4, dzc, n, CP, c, (float)(m1 / M), (float)(m2 / M));
      }
    }
  }
}

// phase 2 for partial tables with MANY slots per sample (the input-gradient epilogue writes one per (tile, strip): 1100+ at
// 506 x 512): one block per (group, sample) -- N x groups blocks instead of `groups` (the one-block form above walks the
// samples with 16 waves: 62 us for a level-0 layer, latency-bound) -- writes m12[n][g] and the per-(sample, channel) sums
// pc[n][CP][2] = (sum dz, sum dz yhat); dgamma / dbeta are accumulated from pc in sample order by k_gn_param_grads.
// The four waves take a quarter of the slots each and are combined in a fixed order (deterministic).
__global__ __launch_bounds__(256) void k_gn_bwd_finalize_n(const float* __restrict__ part, int blocks, int C, int CP, int groups, int hw,
                                                           const float* __restrict__ gamma, float* __restrict__ m12,
                                                           float* __restrict__ pc, const float* __restrict__ coef4,
                                                           float* __restrict__ dzc) {
  const int g = blockIdx.x, n = blockIdx.y, cpg = C / groups;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double sm[4][16];
  __shared__ float mf[2];
  const int per = (blocks + 3) / 4, b0 = wave * per, cnt = max(0, min(per, blocks - b0));
  double a1, a2;
  group_channel_sums(part, (size_t)n * blocks + b0, cnt, CP, g * cpg, cpg, a1, a2);      // cpg is a power of two <= 8 (host check)
  if (lane < cpg) { sm[wave][2 * lane] = a1; sm[wave][2 * lane + 1] = a2; }
  __syncthreads();
  if (threadIdx.x < 2 * cpg) {
    const double t = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
    pc[((size_t)n * CP + g * cpg + (threadIdx.x >> 1)) * 2 + (threadIdx.x & 1)] = (float)t;
    sm[0][threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x < 2 && m12) {
    double m = 0.0;
    for (int k = 0; k < cpg; ++k) m += (double)(gamma ? gamma[g * cpg + k] : 1.f) * sm[0][2 * k + threadIdx.x];
    m12[((size_t)n * groups + g) * 2 + threadIdx.x] = (float)(m / ((double)cpg * (double)hw));
    mf[threadIdx.x] = (float)(m / ((double)cpg * (double)hw));
  }
  if (dzc) {                                                // (the host passes dzc only together with m12)
    __syncthreads();
    if ((int)threadIdx.x < cpg) write_dz_coef(coef4, dzc, n, CP, g * cpg + threadIdx.x, mf[0], mf[1]);
  }
}

// phase 3: dy = rstd (dz gamma - m1 - yhat m2)   (GN)   |   dy = da act'(y)   (act only)
template <typename T, int GK = 0, typename TY = T, bool DROP = false>
__global__ __launch_bounds__(256) void k_gn_bwd_apply(GnArgs a, const TY* __restrict__ y, const float* __restrict__ m12,
                                                      mc_grad_src g0, mc_grad_src g1, T* __restrict__ dy, int rows_pb, DropK dk) {
  const int n = (int)blockIdx.z, cb = blockIdx.y;
  float sc[8], sh[8], mean[8], rstd[8], ga[8], m1[8], m2[8];
  gn_coef(a, n, cb, sc, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int c = cb * 8 + j;
    mean[j] = 0.f; rstd[j] = 0.f; ga[j] = 0.f; m1[j] = 0.f; m2[j] = 0.f;
    if (c < a.C) {
      if (a.post == MC_POST_GN_ACT) {
        int g = c / a.cpg;
        mean[j] = a.stats[((size_t)n * a.groups + g) * 2];
        rstd[j] = a.stats[((size_t)n * a.groups + g) * 2 + 1];
        ga[j] = a.gamma[c];
        m1[j] = m12[((size_t)n * a.groups + g) * 2];
        m2[j] = m12[((size_t)n * a.groups + g) * 2 + 1];
      } else { ga[j] = 1.f; rstd[j] = 1.f; }
    }
  }
  float cA[8], cB[8], cC[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    cA[j] = rstd[j] * ga[j];                          // (act-only layers: rstd = ga = 1, m1 = m2 = 0)
    cB[j] = -rstd[j] * rstd[j] * m2[j];
    cC[j] = -rstd[j] * m1[j];
  }
  // each block streams GN_ROWS rows: the per-(n, channel-block) coefficient prologue is amortised over several
  // vectors per thread (one vector per thread left these kernels latency-bound at ~1.3 TB/s).  (A 4-way manual batching
  // of the loads was tried and was SLOWER: 131 VGPRs cut the occupancy of this streaming kernel.)
  const int y0 = blockIdx.x * rows_pb, nrows = min(rows_pb, a.H - y0);
  DropSeed sd = {0, 0, 0};
  uint64_t vbase = 0;
  if constexpr (DROP) { sd = drop_seed(dk); vbase = drop_base(n, cb, a.C8, a.H, a.W); }
  for (int i = threadIdx.x; i < nrows * a.W; i += blockDim.x) {      // rows x columns flattened (narrow images)
    const int ry = i / a.W, xx = i - ry * a.W, yy = y0 + ry;
    float v[8], da[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
    size_t idx = cb8_index(n, cb, yy, xx, a.C8, a.H, a.W);
    V8<TY>::ld(y + idx, v);
    grad_fetch_add<T, GKinds<GK>::k0>(g0, n, cb, yy, xx, a.C8, da);
    grad_fetch_add<T, GKinds<GK>::k1>(g1, n, cb, yy, xx, a.C8, da);
    if constexpr (DROP) {
      float ms[8];
      drop_factors(dk, sd, vbase + (uint32_t)(yy * a.W + xx), ms);
#pragma unroll
      for (int j = 0; j < 8; ++j) da[j] *= ms[j];
    }
    float gz[8];
    act_bwd8<FastMath<T>::value>(v, sc, sh, a.act, gz);
    // dy = rstd (gamma dz - m1 - yhat m2) = cA dz + cB (y - mean) + cC  (three packed FMAs per channel pair)
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const f32x2 dz = (f32x2){da[j], da[j + 1]} * (f32x2){gz[j], gz[j + 1]};
      const f32x2 t = (f32x2){v[j], v[j + 1]} - (f32x2){mean[j], mean[j + 1]};
      const f32x2 r = pk_fma((f32x2){cA[j], cA[j + 1]}, dz, pk_fma((f32x2){cB[j], cB[j + 1]}, t, (f32x2){cC[j], cC[j + 1]}));
      o[j] = r.x; o[j + 1] = r.y;
    }
    V8<T>::st(dy + idx, o);
  }
}

// Small layers (levels >= 2 of the U-Net: <= 128 x 128 pixels): the three phases above in ONE launch.  One block per (sample,
// channel block) walks its 8 channels x H x W twice -- sums, block reduction in a fixed order, coefficients, dy -- the second
// walk is served by the caches.  The separate reduce / finalize / apply launches of such a layer take 40-50 us for < 1 MB of
// data: they are bound by launch latency, not by bytes.  Needs every group inside one channel block (channels per group
// 1, 2, 4 or 8).  The per-(sample, channel) sums go to `pc` [N][CP][2]; k_gn_param_grads adds them to dgamma / dbeta in sample
// order for all such layers at the end of the backward pass.
template <typename T, int GK, typename TY = T, bool DROP = false>
__global__ __launch_bounds__(1024) void k_gn_bwd_small(GnArgs a, const TY* __restrict__ y, mc_grad_src g0, mc_grad_src g1,
                                                       T* __restrict__ dy, float* __restrict__ pc, int CP, DropK dk) {
  const int n = (int)blockIdx.y, cb = blockIdx.x;
  float sc[8], sh[8], mean[8], rstd[8], ga[8];
  gn_coef(a, n, cb, sc, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cb * 8 + j;
    mean[j] = 0.f; rstd[j] = 0.f; ga[j] = 0.f;
    if (c < a.C) {
      const int g = c / a.cpg;
      mean[j] = a.stats[((size_t)n * a.groups + g) * 2];
      rstd[j] = a.stats[((size_t)n * a.groups + g) * 2 + 1];
      ga[j] = a.gamma[c];
    }
  }
  const int total = a.H * a.W;
  DropSeed sd = {0, 0, 0};
  uint64_t vbase = 0;
  if constexpr (DROP) { sd = drop_seed(dk); vbase = drop_base(n, cb, a.C8, a.H, a.W); }
  float s[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) s[j] = 0.f;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int yy = i / a.W, xx = i - yy * a.W;
    float v[8], da[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gz[8];
    V8<TY>::ld(y + cb8_index(n, cb, yy, xx, a.C8, a.H, a.W), v);
    grad_fetch_add<T, GKinds<GK>::k0>(g0, n, cb, yy, xx, a.C8, da);
    grad_fetch_add<T, GKinds<GK>::k1>(g1, n, cb, yy, xx, a.C8, da);
    if constexpr (DROP) {                                   // (the same Philox call in both walks: the mask is not kept in registers)
      float ms[8];
      drop_factors(dk, sd, vbase + (uint32_t)i, ms);
#pragma unroll
      for (int j = 0; j < 8; ++j) da[j] *= ms[j];
    }
    act_bwd8<FastMath<T>::value>(v, sc, sh, a.act, gz);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dz = da[j] * gz[j];
      s[2 * j] += dz;
      s[2 * j + 1] += dz * (v[j] - mean[j]) * rstd[j];
    }
  }
  __shared__ float red[16][16];
  __shared__ float tot[16];
  {
    int idx;
    const float r = wave_sum16(s, threadIdx.x & 63, idx);
    if ((threadIdx.x & 3) == 0) red[threadIdx.x >> 6][idx] = r;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    float r = 0.f;
    const int nw = (int)blockDim.x >> 6;
    for (int w = 0; w < nw; ++w) r += red[w][threadIdx.x];          // fixed order: deterministic
    tot[threadIdx.x] = r;
    const int c = cb * 8 + (threadIdx.x >> 1);
    if (c < CP) pc[((size_t)n * CP + c) * 2 + (threadIdx.x & 1)] = r;
  }
  __syncthreads();
  // m1 = sum_c gamma_c s1_c / M, m2 = sum_c gamma_c s2_c / M over the channels of the group (all inside this channel block)
  float cA[8], cB[8], cC[8];
  const float invM = 1.0f / ((float)a.cpg * (float)total);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cb * 8 + j;
    float m1 = 0.f, m2 = 0.f;
    if (c < a.C) {
      const int j0 = (j / a.cpg) * a.cpg;
      for (int k = 0; k < a.cpg; ++k) {
        const float gk = a.gamma[cb * 8 + j0 + k];
        m1 += gk * tot[2 * (j0 + k)];
        m2 += gk * tot[2 * (j0 + k) + 1];
      }
      m1 *= invM; m2 *= invM;
    }
    cA[j] = rstd[j] * ga[j];
    cB[j] = -rstd[j] * rstd[j] * m2;
    cC[j] = -rstd[j] * m1;
  }
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int yy = i / a.W, xx = i - yy * a.W;
    float v[8], da[8] = {0, 0, 0, 0, 0, 0, 0, 0}, gz[8], o[8];
    const size_t idx = cb8_index(n, cb, yy, xx, a.C8, a.H, a.W);
    V8<TY>::ld(y + idx, v);
    grad_fetch_add<T, GKinds<GK>::k0>(g0, n, cb, yy, xx, a.C8, da);
    grad_fetch_add<T, GKinds<GK>::k1>(g1, n, cb, yy, xx, a.C8, da);
    if constexpr (DROP) {                                   // (the same Philox call in both walks: the mask is not kept in registers)
      float ms[8];
      drop_factors(dk, sd, vbase + (uint32_t)i, ms);
#pragma unroll
      for (int j = 0; j < 8; ++j) da[j] *= ms[j];
    }
    act_bwd8<FastMath<T>::value>(v, sc, sh, a.act, gz);
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const f32x2 dz = (f32x2){da[j], da[j + 1]} * (f32x2){gz[j], gz[j + 1]};
      const f32x2 t = (f32x2){v[j], v[j + 1]} - (f32x2){mean[j], mean[j + 1]};
      const f32x2 r = pk_fma((f32x2){cA[j], cA[j + 1]}, dz, pk_fma((f32x2){cB[j], cB[j + 1]}, t, (f32x2){cC[j], cC[j + 1]}));
      o[j] = r.x; o[j + 1] = r.y;
    }
    V8<T>::st(dy + idx, o);
  }
}

// dgamma[c] += sum_n pc[n][c][1], dbeta[c] += sum_n pc[n][c][0], samples in order, for up to GP_MAX layers per launch
constexpr int GP_MAX = 32;
struct GpJob { const float* pc; float* dgamma; float* dbeta; int N, C, CP, first; };
struct GpTable { int n; GpJob j[GP_MAX]; };
__global__ void k_gn_param_grads(GpTable t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int ji = 0;
#pragma unroll 1
  for (int k = 1; k < t.n; ++k) if (i >= t.j[k].first) ji = k;
  const GpJob& j = t.j[ji];
  const int c = i - j.first;
  if (c >= j.C) return;
  float s1 = 0.f, s2 = 0.f;
  for (int n = 0; n < j.N; ++n) { s1 += j.pc[((size_t)n * j.CP + c) * 2]; s2 += j.pc[((size_t)n * j.CP + c) * 2 + 1]; }
  if (j.dgamma) j.dgamma[c] += s2;
  if (j.dbeta) j.dbeta[c] += s1;
}

// The same padding adjoint for a gradient buffer whose non-frame pixels already hold dz = dA * act'(z) (written by the
// input-gradient kernel's epilogue): EVERY frame pixel (within p + 1 of the border; `all`: every pixel) gets its halo
// sources added, is turned into dz in place and contributes to this block's (sum dz, sum dz * yhat) partials
// part[n][stride][CP][2] at slot first + blockIdx.x.  With zero padding there is nothing to fold and no frame.
template <typename T, typename TY = T>
__global__ __launch_bounds__(256) void k_fold_padded_dz(T* __restrict__ buf, int C8, int H, int W, int p, int mode, int all,
                                                        const TY* __restrict__ y, const float* __restrict__ coef4, int act,
                                                        float* __restrict__ part, int stride, int first) {
  const int n = blockIdx.z, cb = blockIdx.y;
  const int t = p + 1;
  const int band = all ? H * W : 2 * t * W;
  const int side = all ? 0 : (H - 2 * t) * 2 * t;
  const int Hp = H + 2 * p, Wp = W + 2 * p, CP = C8 * 8;
  float sc[8], sh[8], me[8], rs[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (coef4) {
      const float4 c4 = reinterpret_cast<const float4*>(coef4)[(size_t)n * CP + cb * 8 + j];
      sc[j] = c4.x; sh[j] = c4.y; me[j] = c4.z; rs[j] = c4.w;
    } else { sc[j] = 1.f; sh[j] = 0.f; me[j] = 0.f; rs[j] = 0.f; }
  }
  float s[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) s[j] = 0.f;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;          // one pixel per thread (the launch covers band + side)
  if (i < band + side) {
    int yy, xx;
    if (all) {
      yy = i / W;
      xx = i - yy * W;
    } else if (i < band) {
      int r = i / W;
      xx = i - r * W;
      yy = r < t ? r : H - 2 * t + r;
    } else {
      int k = i - band;
      int r = k / (2 * t), c = k - r * 2 * t;
      yy = t + r;
      xx = c < t ? c : W - 2 * t + c;
    }
    int cy[6], cx[6];
    const int ny = fold_candidates(yy, H, p, mode, cy), nx = fold_candidates(xx, W, p, mode, cx);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) {
        float v[8];
        V8<T>::ld(buf + cb8_index(n, cb, cy[a], cx[b], C8, Hp, Wp), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
      }
    float yv[8], gz[8];
    V8<TY>::ld(y + cb8_index(n, cb, yy, xx, C8, H, W), yv);
    act_bwd8<FastMath<T>::value>(yv, sc, sh, act, gz);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dz = acc[j] * gz[j];
      acc[j] = dz;
      s[2 * j] = dz;
      s[2 * j + 1] = dz * (yv[j] - me[j]) * rs[j];
    }
    V8<T>::st(buf + cb8_index(n, cb, yy + p, xx + p, C8, Hp, Wp), acc);
  }
  __shared__ float red[4][16];
  int idx;
  float r = wave_sum16(s, threadIdx.x & 63, idx);
  if ((threadIdx.x & 3) == 0) red[threadIdx.x >> 6][idx] = r;
  __syncthreads();
  if (threadIdx.x < 16) {
    float tot = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    part[(((size_t)n * stride + first + blockIdx.x) * CP + cb * 8 + (threadIdx.x >> 1)) * 2 + (threadIdx.x & 1)] = tot;
  }
}

// GroupNorm backward, last phase, from dz (see mc_gn_bwd_apply_dz): dy = scale dz - rstd (m1 + yhat m2); coef4 == NULL
// (activation-only layer): dy = dz.  Rows x columns flattened like k_gn_bwd_apply.
template <typename T, int GK, typename TY = T>
__global__ __launch_bounds__(256) void k_gn_bwd_apply_dz(mc_grad_src gs, const TY* __restrict__ y, int C, int C8, int H, int W,
                                                         int groups, const float* __restrict__ coef4,
                                                         const float* __restrict__ m12, T* __restrict__ dy, int rows_pb) {
  const int n = blockIdx.z, cb = blockIdx.y;
  float cA[8], cB[8], cC[8], me[8];
  const int cpg = C / groups;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cb * 8 + j;
    cA[j] = (c < C) ? 1.f : 0.f; cB[j] = 0.f; cC[j] = 0.f; me[j] = 0.f;
    if (coef4 && c < C) {
      const float4 c4 = reinterpret_cast<const float4*>(coef4)[(size_t)n * C8 * 8 + c];
      const int g = c / cpg;
      const float m1 = m12[((size_t)n * groups + g) * 2], m2 = m12[((size_t)n * groups + g) * 2 + 1];
      cA[j] = c4.x;                     // rstd * gamma
      cB[j] = -c4.w * c4.w * m2;
      cC[j] = -c4.w * m1;
      me[j] = c4.z;
    }
  }
  const int y0 = blockIdx.x * rows_pb, nrows = min(rows_pb, H - y0);
  for (int i = threadIdx.x; i < nrows * W; i += blockDim.x) {
    const int ry = i / W, xx = i - ry * W, yy = y0 + ry;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dz[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
    const size_t idx = cb8_index(n, cb, yy, xx, C8, H, W);
    if (coef4) V8<TY>::ld(y + idx, v);
    grad_fetch_add<T, GK>(gs, n, cb, yy, xx, C8, dz);
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const f32x2 t = (f32x2){v[j], v[j + 1]} - (f32x2){me[j], me[j + 1]};
      const f32x2 r = pk_fma((f32x2){cA[j], cA[j + 1]}, (f32x2){dz[j], dz[j + 1]},
                             pk_fma((f32x2){cB[j], cB[j + 1]}, t, (f32x2){cC[j], cC[j + 1]}));
      o[j] = r.x; o[j + 1] = r.y;
    }
    V8<T>::st(dy + idx, o);
  }
}

}  // namespace

extern "C" {

int mc_gn_partials(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, int32_t tiles, float* part,
                   void* stream) {
  if (!y || !part || n <= 0 || c <= 0 || h <= 0 || w <= 0 || tiles <= 0 || tiles > h) return MC_EINVAL;
  const int C8 = (c + 7) / 8;
  dim3 g(tiles, C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_gn_partials<T>, g, dim3(256), 0, s, (const T*)y, C8, h, w, tiles, part);
  });
}

int mc_gn_finalize_coef(const float* part, int32_t n, int32_t tiles, int32_t c, int32_t groups, int32_t hw, float eps,
                        const float* gamma, const float* beta, float* stats, float* coef4, void* stream) {
  if (!part || n <= 0 || tiles <= 0 || c <= 0 || groups <= 0 || c % groups != 0 || hw <= 0) return MC_EINVAL;
  if (!stats && !coef4) return MC_EINVAL;
  if (coef4 && (!gamma || !beta)) return MC_EINVAL;
  int CP = ((c + 7) / 8) * 8;
  hipLaunchKernelGGL(k_gn_finalize, dim3(groups, n), dim3(64), 0, (hipStream_t)stream, part, tiles, c, CP, groups, hw,
                     eps, stats, nullptr, gamma, beta, coef4);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_gn_finalize(const float* part, int32_t n, int32_t tiles, int32_t c, int32_t groups, int32_t hw, float eps,
                   float* stats, float* chan_mean, void* stream) {
  if (!part || n <= 0 || tiles <= 0 || c <= 0 || groups <= 0 || c % groups != 0 || hw <= 0) return MC_EINVAL;
  if (!stats && !chan_mean) return MC_EINVAL;
  int CP = ((c + 7) / 8) * 8;
  hipLaunchKernelGGL(k_gn_finalize, dim3(groups, n), dim3(64), 0, (hipStream_t)stream, part, tiles, c, CP, groups, hw,
                     eps, stats, chan_mean, nullptr, nullptr, nullptr);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

static int fill_gn_args(GnArgs& a, int n, int c, int h, int w, int groups, const float* stats, const float* gamma,
                        const float* beta, int post, int act) {
  if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MC_EINVAL;
  if (post == MC_POST_GN_ACT && (groups <= 0 || c % groups != 0 || !stats || !gamma || !beta)) return MC_EINVAL;
  if (post < MC_POST_NONE || post > MC_POST_GN_ACT || act < MC_ACT_NONE || act > MC_ACT_ELU) return MC_EINVAL;
  a.N = n; a.C = c; a.C8 = (c + 7) / 8; a.H = h; a.W = w;
  a.groups = groups > 0 ? groups : 1;
  a.cpg = c / a.groups; a.post = post; a.act = act;
  a.stats = stats; a.gamma = gamma; a.beta = beta;
  return MC_OK;
}

// dropout descriptor of the C ABI -> kernel argument (drop == NULL: the plain kernels; *ok = 0 on a malformed descriptor)
static DropK drop_args(const mc_dropout* d, int* ok) {
  DropK k = {nullptr, 0u, 0u, 0.f};
  *ok = 1;
  if (!d) return k;
  if (!d->state || d->keep16 < 1u || d->keep16 > 65535u) { *ok = 0; return k; }
  k.state = d->state; k.layer = d->layer; k.keep16 = d->keep16;
  k.scale = (float)(65536.0 / (double)d->keep16);
  return k;
}

static int gn_act_fwd(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                      const float* gamma, const float* beta, int32_t post, int32_t act, int32_t pool, int32_t dtype,
                      void* a_out, void* pooled, const mc_dropout* drop, void* stream) {
  GnArgs a;
  int rc = fill_gn_args(a, n, c, h, w, groups, stats, gamma, beta, post, act);
  if (rc) return rc;
  int dok;
  const DropK dk = drop_args(drop, &dok);
  if (!dok) return MC_EINVAL;
  if (drop && pool != 1) return MC_EUNSUPPORTED;
  if (!y || (!a_out && pool == 1) || (pool > 1 && !pooled)) return MC_EINVAL;
  if (pool != 1 && pool != 2 && pool != 4) return MC_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int per = cdiv(h, pool) * cdiv(w, pool);
  dim3 g(max(1, min(cdiv(per, 256 * gn_fwd_vpt()), 4096)), a.C8, n);
  if (pool == 2 && (w & 1) == 0 && h >= 2 && dtype != MC_F32) {     // row-pair form (16-bit types: one 16-byte vector per pixel)
    dim3 gp(max(1, min(cdiv(cdiv(h, 2) * w, 256 * 2), 4096)), a.C8, n);
    if (dtype == MC_BF16) hipLaunchKernelGGL(k_gn_act_fwd_pool2_rows<bf16_t>, gp, dim3(256), 0, s, a, (const bf16_t*)y, (bf16_t*)a_out, (bf16_t*)pooled);
    else if (dtype == MC_MIX16) hipLaunchKernelGGL(k_gn_act_fwd_pool2_rows<f16_t>, gp, dim3(256), 0, s, a, (const f16_t*)y, (f16_t*)a_out, (f16_t*)pooled);
    else return MC_EUNSUPPORTED;
    MC_CHECK_LAUNCH();
    return MC_OK;
  }
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, a, (const T*)y, (T*)a_out, (T*)pooled, dk); };
    if (drop) launch(k_gn_act_fwd<T, 1, true>);
    else if (pool == 1) launch(k_gn_act_fwd<T, 1>);
    else if (pool == 2) launch(k_gn_act_fwd<T, 2>);
    else launch(k_gn_act_fwd<T, 4>);
  });
}
int mc_gn_act_fwd(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                  const float* gamma, const float* beta, int32_t post, int32_t act, int32_t pool, int32_t dtype,
                  void* a_out, void* pooled, void* stream) {
  return gn_act_fwd(y, n, c, h, w, groups, stats, gamma, beta, post, act, pool, dtype, a_out, pooled, nullptr, stream);
}
int mc_gn_act_fwd_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                       const float* gamma, const float* beta, int32_t post, int32_t act, int32_t pool, int32_t dtype,
                       void* a_out, void* pooled, const mc_dropout* drop, void* stream) {
  if (!drop) return MC_EINVAL;
  return gn_act_fwd(y, n, c, h, w, groups, stats, gamma, beta, post, act, pool, dtype, a_out, pooled, drop, stream);
}

int32_t mc_gn_bwd_blocks(int32_t h, int32_t w) {
  static int env_vpt = env_int("MC_GN_RED_VPT", 0);
  // vectors per thread of the phase-1 reduction.  Round 2 used 32 on large images (measured on the kernel alone); inside the
  // round-3 step 8 is better everywhere (whole step at 32 x 506 x 512, 8 / 16 / 32 / 64: 10.15 / 10.19 / 10.33 / 10.57 ms
  // mixed, 10.10 / 10.10 / 10.31 plain bf16: the two-source reduction of the encoder's last layers wants many short blocks)
  const int vpt = env_vpt > 0 ? env_vpt : 8;
  int b = cdiv(h * w, 256 * vpt);
  if (b > 128) b = 128;
  if (b < 1) b = 1;
  return b;
}

static int gn_act_bwd_reduce(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                             const float* gamma, const float* beta, int32_t post, int32_t act, int32_t dtype,
                             const mc_grad_src* g0, const mc_grad_src* g1, float* partials, const mc_dropout* drop, void* stream) {
  GnArgs a;
  int rc = fill_gn_args(a, n, c, h, w, groups, stats, gamma, beta, post, act);
  if (rc) return rc;
  int dok;
  const DropK dk = drop_args(drop, &dok);
  if (!dok) return MC_EINVAL;
  if (post != MC_POST_GN_ACT || !y || !partials || !g0) return MC_EINVAL;
  if ((rc = check_gsrc(g0)) || (rc = check_gsrc(g1))) return rc;
  dim3 g(mc_gn_bwd_blocks(h, w), a.C8, n);
  hipStream_t s = (hipStream_t)stream;
  const mc_grad_src s0 = gsrc_or_none(g0), s1 = gsrc_or_none(g1);
  return with_gn_bwd_variant(dtype, gkind_of(s0, s1), drop != nullptr, [&](auto t, auto ty, auto gk, auto dr) {
    using T = typename decltype(t)::type; using TY = typename decltype(ty)::type;
    hipLaunchKernelGGL((k_gn_bwd_reduce<T, decltype(gk)::value, TY, decltype(dr)::value>), g, dim3(256), 0, s, a, (const TY*)y, s0, s1,
                       partials, a.C8 * 8, dk);
  });
}
int mc_gn_act_bwd_reduce(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                         const float* gamma, const float* beta, int32_t post, int32_t act, int32_t dtype,
                         const mc_grad_src* g0, const mc_grad_src* g1, float* partials, void* stream) {
  return gn_act_bwd_reduce(y, n, c, h, w, groups, stats, gamma, beta, post, act, dtype, g0, g1, partials, nullptr, stream);
}
int mc_gn_act_bwd_reduce_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                              const float* gamma, const float* beta, int32_t post, int32_t act, int32_t dtype,
                              const mc_grad_src* g0, const mc_grad_src* g1, float* partials, const mc_dropout* drop,
                              void* stream) {
  if (!drop) return MC_EINVAL;
  return gn_act_bwd_reduce(y, n, c, h, w, groups, stats, gamma, beta, post, act, dtype, g0, g1, partials, drop, stream);
}

int mc_gn_act_bwd_finalize(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                           const float* gamma, float* m12, float* dgamma, float* dbeta, void* stream) {
  if (!partials || n <= 0 || blocks <= 0 || c <= 0 || groups <= 0 || c % groups || hw <= 0) return MC_EINVAL;
  hipLaunchKernelGGL(k_gn_bwd_finalize, dim3(groups), dim3(1024), 0, (hipStream_t)stream, partials, n, blocks, c,
                     ((c + 7) / 8) * 8, groups, hw, gamma, m12, dgamma, dbeta, (const float*)nullptr, (float*)nullptr);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_gn_act_bwd_finalize_n(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                             const float* gamma, float* m12, float* chan_sums, void* stream) {
  if (!partials || !chan_sums || n <= 0 || blocks <= 0 || c <= 0 || groups <= 0 || c % groups || hw <= 0) return MC_EINVAL;
  const int cpg = c / groups;
  if (cpg != 1 && cpg != 2 && cpg != 4 && cpg != 8) return MC_EUNSUPPORTED;
  hipLaunchKernelGGL(k_gn_bwd_finalize_n, dim3(groups, n), dim3(256), 0, (hipStream_t)stream, partials, blocks, c,
                     ((c + 7) / 8) * 8, groups, hw, gamma, m12, chan_sums, (const float*)nullptr, (float*)nullptr);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_gn_act_bwd_finalize_dz(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                              const float* gamma, float* m12, float* dgamma, float* dbeta, const float* coef, float* dz_coef,
                              void* stream) {
  if (!partials || !m12 || !coef || !dz_coef || n <= 0 || blocks <= 0 || c <= 0 || groups <= 0 || c % groups || hw <= 0) return MC_EINVAL;
  hipLaunchKernelGGL(k_gn_bwd_finalize, dim3(groups), dim3(1024), 0, (hipStream_t)stream, partials, n, blocks, c,
                     ((c + 7) / 8) * 8, groups, hw, gamma, m12, dgamma, dbeta, coef, dz_coef);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_gn_act_bwd_finalize_n_dz(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                                const float* gamma, float* m12, float* chan_sums, const float* coef, float* dz_coef,
                                void* stream) {
  if (!partials || !chan_sums || !m12 || !coef || !dz_coef || n <= 0 || blocks <= 0 || c <= 0 || groups <= 0 || c % groups || hw <= 0)
    return MC_EINVAL;
  const int cpg = c / groups;
  if (cpg != 1 && cpg != 2 && cpg != 4 && cpg != 8) return MC_EUNSUPPORTED;
  hipLaunchKernelGGL(k_gn_bwd_finalize_n, dim3(groups, n), dim3(256), 0, (hipStream_t)stream, partials, blocks, c,
                     ((c + 7) / 8) * 8, groups, hw, gamma, m12, chan_sums, coef, dz_coef);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

static int gn_act_bwd_apply(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                            const float* m12, const float* gamma, const float* beta, int32_t post, int32_t act,
                            int32_t dtype, const mc_grad_src* g0, const mc_grad_src* g1, void* dy, const mc_dropout* drop,
                            void* stream) {
  GnArgs a;
  int rc = fill_gn_args(a, n, c, h, w, groups, stats, gamma, beta, post, act);
  if (rc) return rc;
  int dok;
  const DropK dk = drop_args(drop, &dok);
  if (!dok) return MC_EINVAL;
  if (!y || !dy || !g0 || (post == MC_POST_GN_ACT && !m12)) return MC_EINVAL;
  if ((rc = check_gsrc(g0)) || (rc = check_gsrc(g1))) return rc;
  if (post == MC_POST_NONE) a.act = MC_ACT_NONE;
  const int rows = gn_apply_rows(h, w);
  dim3 g(cdiv(h, rows), a.C8, n);
  hipStream_t s = (hipStream_t)stream;
  const mc_grad_src s0 = gsrc_or_none(g0), s1 = gsrc_or_none(g1);
  return with_gn_bwd_variant(dtype, gkind_of(s0, s1), drop != nullptr, [&](auto t, auto ty, auto gk, auto dr) {
    using T = typename decltype(t)::type; using TY = typename decltype(ty)::type;
    hipLaunchKernelGGL((k_gn_bwd_apply<T, decltype(gk)::value, TY, decltype(dr)::value>), g, dim3(256), 0, s, a, (const TY*)y, m12, s0, s1,
                       (T*)dy, rows, dk);
  });
}
int mc_gn_act_bwd_apply(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                        const float* m12, const float* gamma, const float* beta, int32_t post, int32_t act,
                        int32_t dtype, const mc_grad_src* g0, const mc_grad_src* g1, void* dy, void* stream) {
  return gn_act_bwd_apply(y, n, c, h, w, groups, stats, m12, gamma, beta, post, act, dtype, g0, g1, dy, nullptr, stream);
}
int mc_gn_act_bwd_apply_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                             const float* m12, const float* gamma, const float* beta, int32_t post, int32_t act,
                             int32_t dtype, const mc_grad_src* g0, const mc_grad_src* g1, void* dy, const mc_dropout* drop,
                             void* stream) {
  if (!drop) return MC_EINVAL;
  return gn_act_bwd_apply(y, n, c, h, w, groups, stats, m12, gamma, beta, post, act, dtype, g0, g1, dy, drop, stream);
}

static int gn_act_fwd_small(const void* y, const float* stat_partials, int32_t tiles, int32_t n, int32_t c, int32_t h, int32_t w,
                            int32_t groups, float eps, const float* gamma, const float* beta, int32_t act, int32_t pool,
                            int32_t dtype, float* stats_out, void* a_out, void* pooled, const mc_dropout* drop, void* stream) {
  GnArgs a;
  int rc = fill_gn_args(a, n, c, h, w, groups, stats_out, gamma, beta, MC_POST_GN_ACT, act);
  if (rc) return rc;
  int dok;
  const DropK dk = drop_args(drop, &dok);
  if (!dok) return MC_EINVAL;
  if (drop && pool != 1) return MC_EUNSUPPORTED;
  if (!y || !stat_partials || tiles <= 0 || !gamma || !beta || !stats_out || !a_out || (pool > 1 && !pooled)) return MC_EINVAL;
  if (pool != 1 && pool != 2) return MC_EUNSUPPORTED;
  if (a.cpg != 1 && a.cpg != 2 && a.cpg != 4 && a.cpg != 8) return MC_EUNSUPPORTED;
  dim3 g(a.C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, g, dim3(gn_small_threads(a.C8 * n)), 0, s, a, (const T*)y, stat_partials, tiles, eps, stats_out, (T*)a_out,
                         (T*)pooled, dk);
    };
    if (drop) launch(k_gn_act_small<T, 1, true>);
    else if (pool == 1) launch(k_gn_act_small<T, 1>);
    else launch(k_gn_act_small<T, 2>);
  });
}
int mc_gn_act_fwd_small(const void* y, const float* stat_partials, int32_t tiles, int32_t n, int32_t c, int32_t h, int32_t w,
                        int32_t groups, float eps, const float* gamma, const float* beta, int32_t act, int32_t pool,
                        int32_t dtype, float* stats_out, void* a_out, void* pooled, void* stream) {
  return gn_act_fwd_small(y, stat_partials, tiles, n, c, h, w, groups, eps, gamma, beta, act, pool, dtype, stats_out, a_out, pooled,
                          nullptr, stream);
}
int mc_gn_act_fwd_small_drop(const void* y, const float* stat_partials, int32_t tiles, int32_t n, int32_t c, int32_t h, int32_t w,
                             int32_t groups, float eps, const float* gamma, const float* beta, int32_t act, int32_t pool,
                             int32_t dtype, float* stats_out, void* a_out, void* pooled, const mc_dropout* drop, void* stream) {
  if (!drop) return MC_EINVAL;
  return gn_act_fwd_small(y, stat_partials, tiles, n, c, h, w, groups, eps, gamma, beta, act, pool, dtype, stats_out, a_out, pooled,
                          drop, stream);
}

static int gn_act_bwd_small(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                            const float* gamma, const float* beta, int32_t act, int32_t dtype, const mc_grad_src* g0,
                            const mc_grad_src* g1, void* dy, float* chan_sums, const mc_dropout* drop, void* stream) {
  GnArgs a;
  int rc = fill_gn_args(a, n, c, h, w, groups, stats, gamma, beta, MC_POST_GN_ACT, act);
  if (rc) return rc;
  int dok;
  const DropK dk = drop_args(drop, &dok);
  if (!dok) return MC_EINVAL;
  if (!y || !dy || !g0 || !stats || !gamma || !beta || !chan_sums) return MC_EINVAL;
  if (a.cpg != 1 && a.cpg != 2 && a.cpg != 4 && a.cpg != 8) return MC_EUNSUPPORTED;     // a group must lie inside one channel block
  if ((rc = check_gsrc(g0)) || (rc = check_gsrc(g1))) return rc;
  dim3 g(a.C8, n);
  hipStream_t s = (hipStream_t)stream;
  const mc_grad_src s0 = gsrc_or_none(g0), s1 = gsrc_or_none(g1);
  const int CP = a.C8 * 8;
  return with_gn_bwd_variant(dtype, gkind_of(s0, s1), drop != nullptr, [&](auto t, auto ty, auto gk, auto dr) {
    using T = typename decltype(t)::type; using TY = typename decltype(ty)::type;
    hipLaunchKernelGGL((k_gn_bwd_small<T, decltype(gk)::value, TY, decltype(dr)::value>), g, dim3(gn_small_threads(a.C8 * n)), 0, s, a,
                       (const TY*)y, s0, s1, (T*)dy, chan_sums, CP, dk);
  });
}
int mc_gn_act_bwd_small(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                        const float* gamma, const float* beta, int32_t act, int32_t dtype, const mc_grad_src* g0,
                        const mc_grad_src* g1, void* dy, float* chan_sums, void* stream) {
  return gn_act_bwd_small(y, n, c, h, w, groups, stats, gamma, beta, act, dtype, g0, g1, dy, chan_sums, nullptr, stream);
}
int mc_gn_act_bwd_small_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats,
                             const float* gamma, const float* beta, int32_t act, int32_t dtype, const mc_grad_src* g0,
                             const mc_grad_src* g1, void* dy, float* chan_sums, const mc_dropout* drop, void* stream) {
  if (!drop) return MC_EINVAL;
  return gn_act_bwd_small(y, n, c, h, w, groups, stats, gamma, beta, act, dtype, g0, g1, dy, chan_sums, drop, stream);
}

// ---- dropout state and the host twins of the generator (csrc/philox.h) -------------------------
__global__ void k_dropout_advance(uint32_t* __restrict__ state) { state[2] += 1u; }

int mc_dropout_advance(uint32_t* state, void* stream) {
  if (!state) return MC_EINVAL;
  hipLaunchKernelGGL(k_dropout_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, state);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

void mc_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t o[4];
  mc_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], o);
  for (int i = 0; i < 4; ++i) out[i] = o[i];
}

int mc_dropout_mask_host(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t layer, uint64_t first_vec, uint64_t n_vec,
                         uint32_t keep16, uint8_t* out) {
  if (!out || keep16 < 1u || keep16 > 65535u) return MC_EINVAL;
  for (uint64_t i = 0; i < n_vec; ++i) {
    const uint32_t bits = mc_dropout_keep8(seed_lo, seed_hi, step, layer, first_vec + i, keep16);
    for (int j = 0; j < 8; ++j) out[i * 8 + j] = (uint8_t)((bits >> j) & 1u);
  }
  return MC_OK;
}

int mc_gn_param_grads_batched(const float* const* chan_sums, const int32_t* n, const int32_t* c, float* const* dgamma,
                              float* const* dbeta, int32_t jobs, void* stream) {
  if (!chan_sums || !n || !c || !dgamma || !dbeta || jobs <= 0) return MC_EINVAL;
  for (int base = 0; base < jobs; base += GP_MAX) {
    GpTable t;
    t.n = jobs - base < GP_MAX ? jobs - base : GP_MAX;
    int first = 0;
    for (int k = 0; k < t.n; ++k) {
      const int i = base + k;
      if (!chan_sums[i] || n[i] <= 0 || c[i] <= 0) return MC_EINVAL;
      t.j[k].pc = chan_sums[i]; t.j[k].dgamma = dgamma[i]; t.j[k].dbeta = dbeta[i];
      t.j[k].N = n[i]; t.j[k].C = c[i]; t.j[k].CP = ((c[i] + 7) / 8) * 8; t.j[k].first = first;
      first += ((c[i] + 63) / 64) * 64;
    }
    hipLaunchKernelGGL(k_gn_param_grads, dim3(first / 64), dim3(64), 0, (hipStream_t)stream, t);
  }
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_fold_padded_dz(void* buf, int32_t n, int32_t c, int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode, int32_t dtype,
                      const void* y, const float* coef, int32_t act, float* partials, int32_t part_stride_blocks,
                      int32_t part_first_block, void* stream) {
  if (!buf || !y || !partials || n <= 0 || c <= 0 || hs <= 0 || ws <= 0 || pad < 0 || pad > 2) return MC_EINVAL;
  if (act < MC_ACT_NONE || act > MC_ACT_ELU) return MC_EINVAL;
  const int blocks = mc_fold_blocks(hs, ws, pad, pad_mode);
  if (blocks == 0) return MC_OK;                              // zero padding: every interior pixel was final already
  if (part_first_block < 0 || part_first_block + blocks > part_stride_blocks) return MC_EINVAL;
  int all, total;
  fold_shape(hs, ws, pad, all, total);
  const int C8 = (c + 7) / 8;
  dim3 g(blocks, C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_grad_y_types(dtype, [&](auto t, auto ty) {
    using T = typename decltype(t)::type; using TY = typename decltype(ty)::type;
    hipLaunchKernelGGL((k_fold_padded_dz<T, TY>), g, dim3(256), 0, s, (T*)buf, C8, hs, ws, pad, pad_mode, all, (const TY*)y, coef, act, partials,
                       part_stride_blocks, part_first_block);
  });
}

int mc_gn_bwd_apply_dz(const mc_grad_src* dz, const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                       const float* coef, const float* m12, int32_t dtype, void* dy, void* stream) {
  if (!dz || !dy || n <= 0 || c <= 0 || h <= 0 || w <= 0) return MC_EINVAL;
  if (coef && (!y || !m12 || groups <= 0 || c % groups != 0)) return MC_EINVAL;
  int rc = check_gsrc(dz);
  if (rc) return rc;
  if ((dz->kind != MC_GSRC_PADFOLD && dz->kind != MC_GSRC_PLAIN) || dz->c8_total != 0 || dz->hs != h || dz->ws != w) return MC_EUNSUPPORTED;
  const int rows = gn_apply_rows(h, w), C8 = (c + 7) / 8;
  dim3 g(cdiv(h, rows), C8, n);
  hipStream_t s = (hipStream_t)stream;
  const int gr = groups > 0 ? groups : 1;
  return with_grad_y_types(dtype, [&](auto t, auto ty) {
    using T = typename decltype(t)::type; using TY = typename decltype(ty)::type;
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, *dz, (const TY*)y, c, C8, h, w, gr, coef, m12, (T*)dy, rows); };
    if (dz->kind == MC_GSRC_PADFOLD) launch(k_gn_bwd_apply_dz<T, MC_GSRC_PADFOLD, TY>);
    else launch(k_gn_bwd_apply_dz<T, MC_GSRC_PLAIN, TY>);
  });
}

}  // extern "C"

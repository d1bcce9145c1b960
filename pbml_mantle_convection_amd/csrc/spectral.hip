// SpectralConv2d (reference pytorch_networks_convae.py:571-635) as a truncated DFT: only the 8 x 4 modes
//   K1 = (0, 1, 2, 3, H-4, H-3, H-2, H-1) x K2 = (0, 1, 2, 3)
// of rfft2 survive the layer, so the transform pair is two streaming kernels over the CB8 tensor and the channel
// mixing is a few thousand complex multiply-adds per sample in mode space.
//
//   analysis   A(t)[n,c,k1,k2] = sum_{h,w} t[n,c,h,w] e^{-i theta}      theta = 2 pi (k1 h / H + k2 w / W)
//   synthesis  S(C)[n,c,h,w]   = sum_{k1,k2} Re(C[n,c,k1,k2] e^{+i theta})
//   forward    y = S(gamma * sum_i A(x)[n,i,.] Wt[i,o,.])                gamma[k2] = (1, 2, 2, 2) / (H W)
//   backward   G = gamma A(dy);  dWt[i,o,.] += sum_n conj(Xhat[n,i,.]) G[n,o,.];  dx = S(sum_o conj(Wt[i,o,.]) G[n,o,.])
//
// Launch shape of both streaming kernels: thread = one column of a 256-column strip, block = strip x chunk of `rpc` rows
// of one (sample, channel block); slot = chunk * strips + strip.  Real input makes the +-k1 column sums conjugates: the
// row walk keeps 9 real accumulators per channel (DC, cos and sin for |k1| = 1..4), the column twiddle and the reduction
// over the strip's columns happen once per block.  Twiddles are f32 tables built on the host in f64 from integer-reduced
// arguments (engine.spectral_tables): rowtw [H][5][2] = (cos, sin)(2 pi (k h mod H) / H), k = 0..4, coltw [W][4][2].
//
// Determinism: no atomics; every combine is a fixed tree or an ordered loop.
// Rounding count (f32 roundings on the longest path from one product to an output element), rpc = rows per chunk:
//   analysis: rpc (row chain of FMAs) + 1 (column twiddle product) + 6 (wave tree) + 3 (four waves in order) + 1 (+-k1)
//   mode space: slots summed in f64, 1 rounding (Xhat as f32); gamma formed in f32 (sp_gamma), 1 rounding; channel mixing in
//   f64, 1 rounding (coefficients as f32)
//   synthesis: 8 (four k2 terms, product + FMA each) + 1 (+-k1 fold) + 8 (row FMAs)
//   = rpc + 31: 63 at rpc = 32 (every grid up to 64 slots of 32 x 256), at most 159 (rpc <= 128, mc_spectral_slots).
#include "common.h"

#define SP_SW 256          // columns per strip = threads per block
#define SP_MODES 32        // 8 x 4 complex modes per channel

static int sp_geometry(int h, int w, int& rpc, int& strips) {
  if (h < 8 || w < 8) return -1;
  strips = cdiv(w, SP_SW);
  rpc = 32;
  while (cdiv(h, rpc) * strips > 64 && rpc < 128) rpc += 32;
  const int slots = cdiv(h, rpc) * strips;
  return slots > 64 ? -1 : slots;
}

int32_t mc_spectral_slots(int32_t h, int32_t w) {
  int rpc, strips;
  return sp_geometry(h, w, rpc, strips);
}

// ---- analysis -----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SP_SW) void k_spectral_analyze(const T* __restrict__ x, int C8, int H, int W, int rpc, int strips,
                                                            int slots, const float* __restrict__ rowtw,
                                                            const float* __restrict__ coltw, float* __restrict__ part) {
  const int slot = blockIdx.x, cb = blockIdx.y, n = blockIdx.z;
  const int chunk = slot / strips, strip = slot - chunk * strips;
  const int xx = strip * SP_SW + threadIdx.x;
  const bool live = xx < W;
  const int y0 = chunk * rpc, y1 = min(H, y0 + rpc);
  float a[5][8], b[5][8];      // a[k] = sum_y t cos(2 pi k y / H), b[k] = sum_y t sin(2 pi k y / H)
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) { a[k][j] = 0.f; b[k][j] = 0.f; }
  const T* p = x + cb8_index(n, cb, y0, live ? xx : 0, C8, H, W);
  for (int y = y0; y < y1; ++y, p += (size_t)W * 8) {
    float v[8];
    if (live) {
      V8<T>::ld(p, v);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    const float* tw = rowtw + (size_t)y * 10;      // block-uniform
#pragma unroll
    for (int j = 0; j < 8; ++j) a[0][j] += v[j];
#pragma unroll
    for (int k = 1; k < 5; ++k) {
      const float c = tw[2 * k], s = tw[2 * k + 1];
#pragma unroll
      for (int j = 0; j < 8; ++j) { a[k][j] = fmaf(v[j], c, a[k][j]); b[k][j] = fmaf(v[j], s, b[k][j]); }
    }
  }
  // column twiddle, then the sum over the strip's columns: per (channel, |k1|, k2) the four real sums
  //   P0 = sum a c2, P1 = sum b s2, P2 = sum a s2, P3 = sum b c2
  float c2[4], s2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c2[q] = live ? coltw[(size_t)xx * 8 + 2 * q] : 0.f;
    s2[q] = live ? coltw[(size_t)xx * 8 + 2 * q + 1] : 0.f;
  }
  __shared__ float red[4][8 * 5 * 16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float s[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        s[4 * q + 0] = a[k][j] * c2[q];
        s[4 * q + 1] = b[k][j] * s2[q];
        s[4 * q + 2] = a[k][j] * s2[q];
        s[4 * q + 3] = b[k][j] * c2[q];
      }
      int idx;
      const float r = wave_sum16(s, lane, idx);
      if ((lane & 3) == 0) red[wave][(j * 5 + k) * 16 + idx] = r;
    }
  }
  __syncthreads();
  // X(+k, k2) = sum (a - i b)(c2 - i s2) = (P0 - P1) + i (-P2 - P3);   X(-k, k2) = sum (a + i b)(c2 - i s2) = (P0 + P1) + i (-P2 + P3)
  const int CP = C8 * 8;
  for (int q = threadIdx.x; q < 8 * SP_MODES * 2; q += SP_SW) {
    const int j = q >> 6, k1i = (q >> 3) & 7, k2 = (q >> 1) & 3, im = q & 1;
    const int k = k1i < 4 ? k1i : 8 - k1i;
    const bool neg = k1i >= 4;
    const int base = (j * 5 + k) * 16 + k2 * 4;
    float P[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) P[i] = ((red[0][base + i] + red[1][base + i]) + red[2][base + i]) + red[3][base + i];
    float v;
    if (!im) v = neg ? P[0] + P[1] : P[0] - P[1];
    else v = neg ? P[3] - P[2] : -P[2] - P[3];
    part[((((size_t)n * slots + slot) * CP + cb * 8 + j) * SP_MODES + k1i * 4 + k2) * 2 + im] = v;
  }
}

int mc_spectral_analyze(const void* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, const float* rowtw,
                        const float* coltw, float* part, void* stream) {
  if (!x || !rowtw || !coltw || !part || n <= 0 || c <= 0) return MC_EINVAL;
  int rpc, strips;
  const int slots = sp_geometry(h, w, rpc, strips);
  if (slots <= 0) return MC_EUNSUPPORTED;
  const int C8 = (c + 7) / 8;
  dim3 g(slots, C8, n);
  hipStream_t s = (hipStream_t)stream;
#define SPA(T) hipLaunchKernelGGL(k_spectral_analyze<T>, g, dim3(SP_SW), 0, s, (const T*)x, C8, h, w, rpc, strips, slots, rowtw, coltw, part)
  if (dtype == MC_F32) SPA(float);
  else if (dtype == MC_BF16) SPA(bf16_t);
  else if (dtype == MC_MIX16) SPA(f16_t);
  else return MC_EUNSUPPORTED;
#undef SPA
  MC_CHECK_LAUNCH();
  return MC_OK;
}

// ---- synthesis ----------------------------------------------------------------------------------------------------
// coef: [n][CP][8][4][2] f32.  y = U0 + sum_{k=1..4} (cos(phi_k) U_k - sin(phi_k) V_k), phi_k = 2 pi k h / H, where with
// E(k1) = sum_k2 coef[k1][k2] e^{+2 pi i k2 w / W}:  U0 = Re E(0);  U_k = Re E(k) + Re E(-k), V_k = Im E(k) - Im E(-k) for
// k = 1..3;  U_4 = Re E(-4), V_4 = -Im E(-4) (the reference's second block starts at H - 4).
template <typename T, bool PART>
__global__ __launch_bounds__(SP_SW) void k_spectral_synthesize(const float* __restrict__ coef, int C, int C8, int H, int W, int rpc,
                                                               int strips, int slots, const float* __restrict__ rowtw,
                                                               const float* __restrict__ coltw, T* __restrict__ y,
                                                               float* __restrict__ part) {
  const int slot = blockIdx.x, cb = blockIdx.y, n = blockIdx.z;
  const int chunk = slot / strips, strip = slot - chunk * strips;
  const int xx = strip * SP_SW + threadIdx.x;
  const bool live = xx < W;
  const int y0 = chunk * rpc, y1 = min(H, y0 + rpc);
  const int CP = C8 * 8;
  float c2[4], s2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    c2[q] = live ? coltw[(size_t)xx * 8 + 2 * q] : 0.f;
    s2[q] = live ? coltw[(size_t)xx * 8 + 2 * q + 1] : 0.f;
  }
  float U[5][8], V[5][8];
  const float* cp = coef + ((size_t)n * CP + cb * 8) * (SP_MODES * 2);      // block-uniform
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool real_ch = cb * 8 + j < C;      // lanes past c stay exactly zero
    float er[8], ei[8];
#pragma unroll
    for (int k1i = 0; k1i < 8; ++k1i) {
      float r = 0.f, i = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float dr = real_ch ? cp[(j * SP_MODES + k1i * 4 + q) * 2] : 0.f;
        const float di = real_ch ? cp[(j * SP_MODES + k1i * 4 + q) * 2 + 1] : 0.f;
        r = fmaf(dr, c2[q], r); r = fmaf(-di, s2[q], r);
        i = fmaf(dr, s2[q], i); i = fmaf(di, c2[q], i);
      }
      er[k1i] = r; ei[k1i] = i;
    }
    U[0][j] = er[0]; V[0][j] = 0.f;
#pragma unroll
    for (int k = 1; k < 4; ++k) { U[k][j] = er[k] + er[8 - k]; V[k][j] = ei[k] - ei[8 - k]; }
    U[4][j] = er[4]; V[4][j] = -ei[4];
  }
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  T* p = y + cb8_index(n, cb, y0, live ? xx : 0, C8, H, W);
  for (int yy = y0; yy < y1; ++yy, p += (size_t)W * 8) {
    const float* tw = rowtw + (size_t)yy * 10;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = U[0][j];
#pragma unroll
    for (int k = 1; k < 5; ++k) {
      const float c = tw[2 * k], s = tw[2 * k + 1];
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[j] = fmaf(c, U[k][j], v[j]); v[j] = fmaf(-s, V[k][j], v[j]); }
    }
    if (live) {
      V8<T>::st(p, v);
      if (PART) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { acc[2 * j] += v[j]; acc[2 * j + 1] += v[j] * v[j]; }
      }
    }
  }
  if (PART) {
    __shared__ float red[4][16];
    int idx;
    const float r = wave_sum16(acc, threadIdx.x & 63, idx);
    if ((threadIdx.x & 3) == 0) red[threadIdx.x >> 6][idx] = r;
    __syncthreads();
    if (threadIdx.x < 16) {
      const float tot = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
      part[(((size_t)n * slots + slot) * CP + cb * 8 + (threadIdx.x >> 1)) * 2 + (threadIdx.x & 1)] = tot;
    }
  }
}

int mc_spectral_synthesize(const float* coef, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, const float* rowtw,
                           const float* coltw, void* y, float* gn_part, void* stream) {
  if (!coef || !rowtw || !coltw || !y || n <= 0 || c <= 0) return MC_EINVAL;
  int rpc, strips;
  const int slots = sp_geometry(h, w, rpc, strips);
  if (slots <= 0) return MC_EUNSUPPORTED;
  const int C8 = (c + 7) / 8;
  dim3 g(slots, C8, n);
  hipStream_t s = (hipStream_t)stream;
#define SPS(T, P) hipLaunchKernelGGL((k_spectral_synthesize<T, P>), g, dim3(SP_SW), 0, s, coef, c, C8, h, w, rpc, strips, slots, rowtw, coltw, (T*)y, gn_part)
#define SPS2(T) do { if (gn_part) SPS(T, true); else SPS(T, false); } while (0)
  if (dtype == MC_F32) SPS2(float);
  else if (dtype == MC_BF16) SPS2(bf16_t);
  else if (dtype == MC_MIX16) SPS2(f16_t);
  else return MC_EUNSUPPORTED;
#undef SPS2
#undef SPS
  MC_CHECK_LAUNCH();
  return MC_OK;
}

// ---- mode space ---------------------------------------------------------------------------------------------------
// Wt[i][o][m], m = k1i * 4 + k2: weights1[i][o][k1i][k2] for k1i < 4, weights2[i][o][k1i - 4][k2] otherwise; both
// [c_i][c_o][4][4] interleaved (re, im) f32, read where the parameters lie.
__device__ __forceinline__ size_t sp_w_index(int i, int o, int m, int c_out) { return (((size_t)i * c_out + o) * 16 + (m & 15)) * 2; }
__device__ __forceinline__ float sp_gamma(int m, int hw) { return ((m & 3) ? 2.0f : 1.0f) / (float)hw; }

// block = one mode m of one sample n.  Phase 1: Xhat[n][i][m] = the slots of the analysis in slot order (f64), kept as f32
// for the backward pass.  Phase 2: coef[n][o][m] = gamma * sum_i Xhat[n][i][m] Wt[i][o][m] in f64; lanes past c_out: zero.
__global__ __launch_bounds__(64) void k_spectral_mix_fwd(const float* __restrict__ part, int slots, int c_in, int CPi, int c_out,
                                                         int CPo, int hw, const float* __restrict__ w1, const float* __restrict__ w2,
                                                         float* __restrict__ xhat, float* __restrict__ coef) {
  const int m = blockIdx.x, n = blockIdx.y;
  for (int i = threadIdx.x; i < CPi; i += blockDim.x) {
    double re = 0.0, im = 0.0;
    if (i < c_in) {
      for (int s = 0; s < slots; ++s) {
        const float* p = part + ((((size_t)n * slots + s) * CPi + i) * SP_MODES + m) * 2;
        re += (double)p[0];
        im += (double)p[1];
      }
    }
    float* q = xhat + (((size_t)n * CPi + i) * SP_MODES + m) * 2;
    q[0] = (float)re;
    q[1] = (float)im;
  }
  __syncthreads();      // (a block reads back only what its own threads wrote)
  const float* wt = m < 16 ? w1 : w2;
  const double g = (double)sp_gamma(m, hw);
  for (int o = threadIdx.x; o < CPo; o += blockDim.x) {
    double re = 0.0, im = 0.0;
    if (o < c_out) {
      for (int i = 0; i < c_in; ++i) {
        const float* q = xhat + (((size_t)n * CPi + i) * SP_MODES + m) * 2;
        const float* w = wt + sp_w_index(i, o, m, c_out);
        const double xr = q[0], xi = q[1], wr = w[0], wi = w[1];
        re += xr * wr - xi * wi;
        im += xr * wi + xi * wr;
      }
    }
    float* d = coef + (((size_t)n * CPo + o) * SP_MODES + m) * 2;
    d[0] = (float)(g * re);
    d[1] = (float)(g * im);
  }
}

int mc_spectral_mix_fwd(const float* part, int32_t n, int32_t slots, int32_t c_in, int32_t c_out, int32_t hw, const float* w1,
                        const float* w2, float* xhat, float* coef, void* stream) {
  if (!part || !w1 || !w2 || !xhat || !coef || n <= 0 || slots <= 0 || slots > 64 || c_in <= 0 || c_out <= 0 || hw <= 0)
    return MC_EINVAL;
  const int CPi = (c_in + 7) / 8 * 8, CPo = (c_out + 7) / 8 * 8;
  hipLaunchKernelGGL(k_spectral_mix_fwd, dim3(SP_MODES, n), dim3(64), 0, (hipStream_t)stream, part, slots, c_in, CPi, c_out, CPo, hw,
                     w1, w2, xhat, coef);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

// block = one mode m, all samples.  Phase 1: G[n][o][m] = gamma * (slots of A(dy) in slot order, f64), as f32 in gbuf.
// Phase 2: dWt[i][o][m] += sum_n conj(Xhat[n][i][m]) G[n][o][m], the samples in order (f64), and, when dxcoef is given,
// dxcoef[n][i][m] = sum_o conj(Wt[i][o][m]) G[n][o][m]; lanes past c_in: zero.
__global__ __launch_bounds__(256) void k_spectral_mix_bwd(const float* __restrict__ part, int N, int slots, int c_in, int CPi,
                                                          int c_out, int CPo, int hw, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, const float* __restrict__ xhat,
                                                          float* __restrict__ gbuf, float* __restrict__ dw1, float* __restrict__ dw2,
                                                          float* __restrict__ dxcoef) {
  const int m = blockIdx.x;
  const double g = (double)sp_gamma(m, hw);
  for (int t = threadIdx.x; t < N * c_out; t += blockDim.x) {
    const int n = t / c_out, o = t - n * c_out;
    double re = 0.0, im = 0.0;
    for (int s = 0; s < slots; ++s) {
      const float* p = part + ((((size_t)n * slots + s) * CPo + o) * SP_MODES + m) * 2;
      re += (double)p[0];
      im += (double)p[1];
    }
    float* q = gbuf + (((size_t)n * CPo + o) * SP_MODES + m) * 2;
    q[0] = (float)(g * re);
    q[1] = (float)(g * im);
  }
  __syncthreads();
  const float* wt = m < 16 ? w1 : w2;
  float* dwt = m < 16 ? dw1 : dw2;
  for (int t = threadIdx.x; t < c_in * c_out; t += blockDim.x) {
    const int i = t / c_out, o = t - i * c_out;
    double re = 0.0, im = 0.0;
    for (int n = 0; n < N; ++n) {
      const float* x = xhat + (((size_t)n * CPi + i) * SP_MODES + m) * 2;
      const float* q = gbuf + (((size_t)n * CPo + o) * SP_MODES + m) * 2;
      const double xr = x[0], xi = x[1], gr = q[0], gi = q[1];
      re += xr * gr + xi * gi;      // conj(x) * g
      im += xr * gi - xi * gr;
    }
    float* d = dwt + sp_w_index(i, o, m, c_out);
    d[0] += (float)re;
    d[1] += (float)im;
  }
  if (dxcoef) {
    for (int t = threadIdx.x; t < N * CPi; t += blockDim.x) {
      const int n = t / CPi, i = t - n * CPi;
      double re = 0.0, im = 0.0;
      if (i < c_in) {
        for (int o = 0; o < c_out; ++o) {
          const float* w = wt + sp_w_index(i, o, m, c_out);
          const float* q = gbuf + (((size_t)n * CPo + o) * SP_MODES + m) * 2;
          const double wr = w[0], wi = w[1], gr = q[0], gi = q[1];
          re += wr * gr + wi * gi;      // conj(w) * g
          im += wr * gi - wi * gr;
        }
      }
      float* d = dxcoef + (((size_t)n * CPi + i) * SP_MODES + m) * 2;
      d[0] = (float)re;
      d[1] = (float)im;
    }
  }
}

int mc_spectral_mix_bwd(const float* part, int32_t n, int32_t slots, int32_t c_in, int32_t c_out, int32_t hw, const float* w1,
                        const float* w2, const float* xhat, float* gbuf, float* dw1, float* dw2, float* dxcoef, void* stream) {
  if (!part || !w1 || !w2 || !xhat || !gbuf || !dw1 || !dw2 || n <= 0 || slots <= 0 || slots > 64 || c_in <= 0 || c_out <= 0 ||
      hw <= 0)
    return MC_EINVAL;
  const int CPi = (c_in + 7) / 8 * 8, CPo = (c_out + 7) / 8 * 8;
  hipLaunchKernelGGL(k_spectral_mix_bwd, dim3(SP_MODES), dim3(256), 0, (hipStream_t)stream, part, n, slots, c_in, CPi, c_out, CPo, hw,
                     w1, w2, xhat, gbuf, dw1, dw2, dxcoef);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

// The CB8 layout boundary and the plain data movers: NCHW f32 <-> CB8 packing, plane sums, average pooling, the in-place
// padding fold, rectangle copies, channel concatenation and its gradient gather, sums of gradient sources.  HBM-bound
// streaming kernels: one thread moves one 8-channel vector (32 B f32 / 16 B bf16), consecutive lanes take consecutive pixels.
#include "common.h"
#include "launch.h"

namespace {

// =================================================================================================
// NCHW f32 <-> CB8
// =================================================================================================
// flat index -> (x, y, channel block, sample); 32-bit divisions when the tensor allows it (the three 64-bit div/mod
// pairs were most of the instructions of the boundary-conversion kernels)
__device__ __forceinline__ void split_index(size_t i, bool small, int Wd, int H, int C8, int& xo, int& y, int& cb, int& n) {
  if (small) {
    unsigned r = (unsigned)i;
    xo = (int)(r % (unsigned)Wd); r /= (unsigned)Wd;
    y = (int)(r % (unsigned)H); r /= (unsigned)H;
    cb = (int)(r % (unsigned)C8);
    n = (int)(r / (unsigned)C8);
  } else {
    xo = (int)(i % Wd);
    size_t r = i / Wd;
    y = (int)(r % H); r /= H;
    cb = (int)(r % C8);
    n = (int)(r / C8);
  }
}

template <typename T>
__global__ void k_pack_nchw(const float* __restrict__ x, int N, int C, int SC, int H, int W, int pad_w, int mode,
                            const float* __restrict__ cs, T* __restrict__ out) {
  const int Wp = W + 2 * pad_w, C8 = (C + 7) / 8;
  size_t total = (size_t)N * C8 * H * Wp;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int xo, y, cb, n;
    split_index(i, total <= 0xffffffffull, Wp, H, C8, xo, y, cb, n);
    int xs = pad_map(xo - pad_w, W, mode);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int c = cb * 8 + j;
      v[j] = (c < C && xs >= 0) ? x[(((size_t)n * SC + c) * H + y) * W + xs] * (cs ? cs[c] : 1.f) : 0.f;
    }
    V8<T>::st(out + i * 8, v);
  }
}

template <typename T>
__global__ void k_unpack_nchw(const T* __restrict__ x, int N, int C, int H, int W, int crop,
                              const float* __restrict__ mean_nc, float* __restrict__ out) {
  const int Wo = W - 2 * crop, C8 = (C + 7) / 8;
  size_t total = (size_t)N * C8 * H * Wo;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int xo, y, cb, n;
    split_index(i, total <= 0xffffffffull, Wo, H, C8, xo, y, cb, n);
    float v[8];
    V8<T>::ld(x + cb8_index(n, cb, y, xo + crop, C8, H, W), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int c = cb * 8 + j;
      if (c < C) {
        float m = mean_nc ? mean_nc[n * C + c] : 0.f;
        out[(((size_t)n * C + c) * H + y) * Wo + xo] = v[j] - m;
      }
    }
  }
}

template <typename T>
__global__ void k_pack_grad_nchw(const float* __restrict__ g, int N, int C, int H, int W, int crop,
                                 const float* __restrict__ mean_nc, T* __restrict__ out) {
  const int Wi = W - 2 * crop, C8 = (C + 7) / 8;
  size_t total = (size_t)N * C8 * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    int xo, y, cb, n;
    split_index(i, total <= 0xffffffffull, W, H, C8, xo, y, cb, n);
    int xi = xo - crop;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int c = cb * 8 + j;
      float val = 0.f;
      if (c < C) {
        if (xi >= 0 && xi < Wi) val = g[(((size_t)n * C + c) * H + y) * Wi + xi];
        if (mean_nc) val -= mean_nc[n * C + c];
      }
      v[j] = val;
    }
    V8<T>::st(out + i * 8, v);
  }
}

__global__ __launch_bounds__(1024) void k_sum_hw(const float* __restrict__ x, int hw, float scale, float* __restrict__ out) {
  // one block per plane (deterministic: fixed per-thread strides, ordered combine; round 1 added 64 block partials per
  // plane with float atomics)
  const float* p = x + (size_t)blockIdx.x * hw;
  float s = 0.f;
  if ((hw & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {        // planes are 16-byte aligned: 4 pixels per load
    const float4* p4 = reinterpret_cast<const float4*>(p);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int i = threadIdx.x; i < hw / 4; i += blockDim.x) {
      const float4 v = p4[i];
      s += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
    }
    s = (s + s1) + (s2 + s3);
  } else {
    for (int i = threadIdx.x; i < hw; i += blockDim.x) s += p[i];
  }
  s = wave_sum(s);
  __shared__ float red[16];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += red[k];
    out[blockIdx.x] = t * scale;
  }
}

template <typename T>
__global__ void k_avgpool(const T* __restrict__ x, int C8, int H, int W, int f, T* __restrict__ out) {
  const int Hp = H / f, Wp = W / f;
  const int n = blockIdx.z, cb = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hp * Wp; i += gridDim.x * blockDim.x) {
    int by = i / Wp, bx = i % Wp;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int dy = 0; dy < f; ++dy)
      for (int dx = 0; dx < f; ++dx) {
        float v[8];
        V8<T>::ld(x + cb8_index(n, cb, by * f + dy, bx * f + dx, C8, H, W), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
      }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= 1.0f / (float)(f * f);
    V8<T>::st(out + cb8_index(n, cb, by, bx, C8, Hp, Wp), acc);
  }
}

// in-place adjoint of F.pad on a padded-domain gradient: one thread per border TARGET pixel (a pixel of the
// interior frame of thickness p+1) gathers its halo sources; sources are halo positions only, so no hazards.
// (buf1 / C8a: a second buffer of the same H x W -- the two input-gradient outputs of a convolution over concatenated
// sources -- folded by the same launch: channel blocks >= C8a belong to buf1, which has C8 - C8a of them)
template <typename T>
__global__ void k_fold_padded(T* __restrict__ buf, int C8, int H, int W, int p, int mode, int all, T* __restrict__ buf1, int C8a) {
  const int n = blockIdx.z;
  int cb = blockIdx.y;
  if (buf1 && cb >= C8a) { buf = buf1; cb -= C8a; C8 -= C8a; } else if (buf1) { C8 = C8a; }
  const int t = p + 1;
  const int band = all ? H * W : 2 * t * W;         // top + bottom bands (all columns); tiny images: every pixel
  const int side = all ? 0 : (H - 2 * t) * 2 * t;   // left + right bands of the remaining rows
  const int Hp = H + 2 * p, Wp = W + 2 * p;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < band + side; i += gridDim.x * blockDim.x) {
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
    int ny = fold_candidates(yy, H, p, mode, cy), nx = fold_candidates(xx, W, p, mode, cx);
    if (ny == 1 && nx == 1) continue;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) {
        float v[8];
        V8<T>::ld(buf + cb8_index(n, cb, cy[a], cx[b], C8, Hp, Wp), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
      }
    V8<T>::st(buf + cb8_index(n, cb, yy + p, xx + p, C8, Hp, Wp), acc);
  }
}

template <typename T>
__global__ void k_rect_copy(const T* __restrict__ src, int hs, int ws, int sy, int sx, T* __restrict__ dst, int hd, int wd,
                            int dy, int dx, int rh, int rw, int C8, int accumulate) {
  const int n = blockIdx.z, cb = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rh * rw; i += gridDim.x * blockDim.x) {
    const int r = i / rw, c = i - r * rw;
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (src) V8<T>::ld(src + cb8_index(n, cb, sy + r, sx + c, C8, hs, ws), v);
    T* d = dst + cb8_index(n, cb, dy + r, dx + c, C8, hd, wd);
    if (accumulate) {
      float o[8];
      V8<T>::ld(d, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += o[j];
    }
    V8<T>::st(d, v);
  }
}

// =================================================================================================
// torch.cat along channels of more than two operands; sum of two gradient sources
// =================================================================================================
constexpr int CAT_MAX = 12;
struct CatTable { int n; const void* src[CAT_MAX]; int c8[CAT_MAX]; int first[CAT_MAX + 1]; };
template <typename T>
__global__ void k_concat_cb8(CatTable t, int C8, int HW, T* __restrict__ out) {
  const int n = blockIdx.z, cb = blockIdx.y;
  int k = 0;
#pragma unroll 1
  for (int j = 1; j < t.n; ++j) if (cb >= t.first[j]) k = j;
  const uint4* s = reinterpret_cast<const uint4*>(t.src[k]) + ((size_t)n * t.c8[k] + (cb - t.first[k])) * HW * (sizeof(T) / 2);
  uint4* d = reinterpret_cast<uint4*>(out) + ((size_t)n * C8 + cb) * HW * (sizeof(T) / 2);
  const int total = HW * (int)(sizeof(T) / 2);                    // 16-byte pieces per plane
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) d[i] = s[i];
}
// eight lanes of one (pixel, channel block) as raw bits: U = uint32_t (f32, two 16-byte pieces) or uint16_t (16-bit types,
// one piece).  Bit moves only, so a concat is exact whatever the values.
template <typename U> struct Lanes8;
template <> struct Lanes8<uint32_t> {
  static __device__ __forceinline__ void ld(const uint32_t* p, uint32_t (&o)[8]) {
    const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
  static __device__ __forceinline__ void st(uint32_t* p, const uint32_t (&o)[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(p + 4) = make_uint4(o[4], o[5], o[6], o[7]);
  }
};
template <> struct Lanes8<uint16_t> {
  static __device__ __forceinline__ void ld(const uint16_t* p, uint32_t (&o)[8]) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    o[0] = a.x & 0xffffu; o[1] = a.x >> 16; o[2] = a.y & 0xffffu; o[3] = a.y >> 16;
    o[4] = a.z & 0xffffu; o[5] = a.z >> 16; o[6] = a.w & 0xffffu; o[7] = a.w >> 16;
  }
  static __device__ __forceinline__ void st(uint16_t* p, const uint32_t (&o)[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
  }
};
// w[i] <- w[i + r] (r > 0) or w[i - |r|] (r < 0), |r| < 8, r uniform across the block: three conditional stages with
// constant indices, so the lanes stay in registers (a select chain on a runtime index is folded back into an indexed load
// from a private array, which lands in scratch or LDS)
template <typename V>
__device__ __forceinline__ void lane_shift16(V (&w)[16], int r) {
#pragma unroll
  for (int s = 4; s >= 1; s >>= 1) {
    if (r >= s && (r & s)) {
#pragma unroll
      for (int i = 0; i + s < 16; ++i) w[i] = w[i + s];
    } else if (r <= -s && ((-r) & s)) {
#pragma unroll
      for (int i = 15; i >= s; --i) w[i] = w[i - s];
    }
  }
}

// torch.cat of operands with any channel counts: operand k holds concat channels [off[k], off[k + 1]).  One thread per
// (pixel, output block); the block's eight lanes come from at most two source blocks of each operand it overlaps
// (16-byte loads), the lanes past the last channel are written as zeros.  Which operands and blocks a block reads
// depends on blockIdx.y only, so every branch is uniform.
struct CatAnyTable { int n; const void* src[CAT_MAX]; int off[CAT_MAX + 1]; };
template <typename U>
__global__ __launch_bounds__(256) void k_concat_cb8_any(CatAnyTable t, int C8, int HW, U* __restrict__ out) {
  const int n = blockIdx.z, cb = blockIdx.y, lo = cb * 8;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < CAT_MAX; ++k) {                              // (unrolled: the table is indexed by constants)
      if (k >= t.n) break;
      const int c = t.off[k + 1] - t.off[k], d = lo - t.off[k];     // local channel of lane j: d + j
      if (d >= c || d + 8 <= 0) continue;
      const int sc8 = (c + 7) / 8, sb = max(d, 0) >> 3;
      const U* s = reinterpret_cast<const U*>(t.src[k]);
      uint32_t w0[8], w1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[16];
      Lanes8<U>::ld(s + ((size_t)(n * sc8 + sb) * HW + i) * 8, w0);
      if (sb + 1 < sc8 && min(d + 8, c) > (sb + 1) * 8) Lanes8<U>::ld(s + ((size_t)(n * sc8 + sb + 1) * HW + i) * 8, w1);
#pragma unroll
      for (int j = 0; j < 8; ++j) { w[j] = w0[j]; w[8 + j] = w1[j]; }
      lane_shift16(w, d - sb * 8);                                   // lane j <- local channel d + j
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (d + j >= 0 && d + j < c) v[j] = w[j];
    }
    Lanes8<U>::st(out + ((size_t)(n * C8 + cb) * HW + i) * 8, v);
  }
}

// gradient of one unaligned concat operand: out (plain CB8, c channels) = channels [c_off, c_off + c) of the
// concatenated tensor's gradient source g (c8t blocks); lanes past c are zeros
template <typename T>
__global__ __launch_bounds__(256) void k_cat_grad_gather(mc_grad_src g, int c8t, int c_off, int c, int C8, int H, int W,
                                                         T* __restrict__ out) {
  const int n = blockIdx.z, cb = blockIdx.y;
  const int lo = c_off + cb * 8, sb = lo >> 3, r0 = lo & 7, nv = min(8, c - cb * 8);
  const bool two = r0 + nv > 8;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W; i += gridDim.x * blockDim.x) {
    const int y = i / W, x = i - y * W;
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w[16], v[8];
    grad_fetch_add<T>(g, n, sb, y, x, c8t, a);
    if (two) grad_fetch_add<T>(g, n, sb + 1, y, x, c8t, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) { w[j] = a[j]; w[8 + j] = b[j]; }
    lane_shift16(w, r0);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < nv ? w[j] : 0.0f;
    V8<T>::st(out + cb8_index(n, cb, y, x, C8, H, W), v);
  }
}

template <typename T>
__global__ void k_gsrc_sum(mc_grad_src g0, mc_grad_src g1, int C8, int H, int W, T* __restrict__ out) {
  const int n = blockIdx.z, cb = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W; i += gridDim.x * blockDim.x) {
    const int y = i / W, x = i - y * W;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    grad_fetch_add<T>(g0, n, cb, y, x, C8, acc);
    grad_fetch_add<T>(g1, n, cb, y, x, C8, acc);
    V8<T>::st(out + cb8_index(n, cb, y, x, C8, H, W), acc);
  }
}

}  // namespace

extern "C" {

int mc_pack_nchw(const float* x, int32_t n, int32_t c, int32_t src_c, int32_t h, int32_t w, int32_t pad_w,
                 int32_t pad_mode, const float* chan_scale, int32_t dtype, void* out, void* stream) {
  if (!x || !out || n <= 0 || c <= 0 || src_c < c || h <= 0 || w <= 0 || pad_w < 0) return MC_EINVAL;
  if (pad_mode == MC_PAD_REFLECT && pad_w >= w) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  size_t total = (size_t)n * ((c + 7) / 8) * h * (w + 2 * pad_w);
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_pack_nchw<T>, grid1(total), dim3(256), 0, s, x, n, c, src_c, h, w, pad_w, pad_mode, chan_scale, (T*)out);
  });
}

int mc_unpack_nchw(const void* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t crop_w, const float* mean_nc,
                   int32_t dtype, float* out, void* stream) {
  if (!x || !out || n <= 0 || c <= 0 || h <= 0 || w <= 2 * crop_w || crop_w < 0) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  size_t total = (size_t)n * ((c + 7) / 8) * h * (w - 2 * crop_w);
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_unpack_nchw<T>, grid1(total), dim3(256), 0, s, (const T*)x, n, c, h, w, crop_w, mean_nc, out);
  });
}

int mc_pack_grad_nchw(const float* g, int32_t n, int32_t c, int32_t h, int32_t w, int32_t crop_w, const float* mean_nc,
                      int32_t dtype, void* out, void* stream) {
  if (!g || !out || n <= 0 || c <= 0 || h <= 0 || w <= 2 * crop_w || crop_w < 0) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  size_t total = (size_t)n * ((c + 7) / 8) * h * w;
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_pack_grad_nchw<T>, grid1(total), dim3(256), 0, s, g, n, c, h, w, crop_w, mean_nc, (T*)out);
  });
}

int mc_sum_hw(const float* x, int32_t nc, int32_t hw, float scale, float* out, void* stream) {
  if (!x || !out || nc <= 0 || hw <= 0) return MC_EINVAL;
  hipLaunchKernelGGL(k_sum_hw, dim3(nc), dim3(1024), 0, (hipStream_t)stream, x, hw, scale, out);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_avgpool_fwd(const void* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t f, int32_t dtype, void* out,
                   void* stream) {
  if (!x || !out || n <= 0 || c <= 0 || f < 1 || h < f || w < f) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  int C8 = (c + 7) / 8;
  dim3 g = grid3((h / f) * (w / f), C8, n, 256, 4096);
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_avgpool<T>, g, dim3(256), 0, s, (const T*)x, C8, h, w, f, (T*)out);
  });
}

int mc_fold_padded2(void* buf0, int32_t c0, void* buf1, int32_t c1, int32_t n, int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode,
                    int32_t dtype, void* stream) {
  if (!buf0 || n <= 0 || c0 <= 0 || hs <= 0 || ws <= 0 || pad < 0 || pad > 2 || (buf1 && c1 <= 0)) return MC_EINVAL;
  if (pad == 0 || pad_mode == MC_PAD_ZEROS) return MC_OK;
  const int C8a = (c0 + 7) / 8, C8 = C8a + (buf1 ? (c1 + 7) / 8 : 0);
  int all, total;
  fold_shape(hs, ws, pad, all, total);
  dim3 g(cdiv(total, 256), C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_fold_padded<T>, g, dim3(256), 0, s, (T*)buf0, C8, hs, ws, pad, pad_mode, all, (T*)buf1, C8a);
  });
}

int mc_fold_padded(void* buf, int32_t n, int32_t c, int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode, int32_t dtype,
                   void* stream) {
  if (!buf || c <= 0) return MC_EINVAL;
  return mc_fold_padded2(buf, c, nullptr, 0, n, hs, ws, pad, pad_mode, dtype, stream);
}

int32_t mc_fold_blocks(int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode) {
  if (hs <= 0 || ws <= 0 || pad <= 0 || pad_mode == MC_PAD_ZEROS) return 0;
  int all, total;
  fold_shape(hs, ws, pad, all, total);
  return cdiv(total, 256);
}

int mc_rect_copy(const void* src, int32_t hs, int32_t ws, int32_t sy, int32_t sx, void* dst, int32_t hd, int32_t wd,
                 int32_t dy, int32_t dx, int32_t rh, int32_t rw, int32_t n, int32_t c, int32_t accumulate, int32_t dtype,
                 void* stream) {
  if (!dst || n <= 0 || c <= 0 || rh <= 0 || rw <= 0) return MC_EINVAL;
  if (dy < 0 || dx < 0 || dy + rh > hd || dx + rw > wd) return MC_EINVAL;
  if (src && (sy < 0 || sx < 0 || sy + rh > hs || sx + rw > ws)) return MC_EINVAL;
  const int C8 = (c + 7) / 8;
  dim3 g(max(1, min(cdiv(rh * rw, 256), 512)), C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_storage_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_rect_copy<T>, g, dim3(256), 0, s, (const T*)src, hs, ws, sy, sx, (T*)dst, hd, wd, dy, dx, rh, rw, C8, accumulate);
  });
}

int mc_concat_cb8(const void* const* srcs, const int32_t* src_c, int32_t n_src, int32_t n, int32_t h, int32_t w,
                  int32_t dtype, void* out, void* stream) {
  if (!srcs || !src_c || !out || n_src < 1 || n_src > CAT_MAX || n <= 0 || h <= 0 || w <= 0) return MC_EINVAL;
  bool aligned = true;                                       // every operand but the last fills whole blocks
  for (int k = 0; k < n_src; ++k) {
    if (!srcs[k] || src_c[k] <= 0) return MC_EINVAL;
    if (k < n_src - 1 && (src_c[k] % 8) != 0) aligned = false;
  }
  if (dtype != MC_F32 && !mc_is16(dtype)) return MC_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (!aligned) {                                            // operand k starts at channel sum_{j<k} C_j
    CatAnyTable t;
    t.n = n_src;
    t.off[0] = 0;
    for (int k = 0; k < n_src; ++k) { t.src[k] = srcs[k]; t.off[k + 1] = t.off[k] + src_c[k]; }
    const int C8 = (t.off[n_src] + 7) / 8;
    dim3 g(max(1, min(cdiv(h * w, 256), 1024)), C8, n);
    if (dtype == MC_F32) hipLaunchKernelGGL(k_concat_cb8_any<uint32_t>, g, dim3(256), 0, s, t, C8, h * w, (uint32_t*)out);
    else hipLaunchKernelGGL(k_concat_cb8_any<uint16_t>, g, dim3(256), 0, s, t, C8, h * w, (uint16_t*)out);
    MC_CHECK_LAUNCH();
    return MC_OK;
  }
  CatTable t;
  t.n = n_src;
  int C8 = 0;
  for (int k = 0; k < n_src; ++k) {
    t.src[k] = srcs[k]; t.c8[k] = (src_c[k] + 7) / 8; t.first[k] = C8;
    C8 += t.c8[k];
  }
  t.first[n_src] = C8;
  const int per = h * w * (dtype == MC_F32 ? 2 : 1);          // (16-bit types: a plain copy of 16-byte pieces)
  dim3 g(max(1, min(cdiv(per, 256 * 4), 1024)), C8, n);
  if (dtype == MC_F32) hipLaunchKernelGGL(k_concat_cb8<float>, g, dim3(256), 0, s, t, C8, h * w, (float*)out);
  else if (mc_is16(dtype)) hipLaunchKernelGGL(k_concat_cb8<bf16_t>, g, dim3(256), 0, s, t, C8, h * w, (bf16_t*)out);
  else return MC_EUNSUPPORTED;
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_cat_grad_gather(const mc_grad_src* g, int32_t c_total, int32_t c_off, int32_t c, int32_t n, int32_t h, int32_t w,
                       int32_t dtype, void* out, void* stream) {
  if (!g || !out || n <= 0 || h <= 0 || w <= 0 || c <= 0 || c_off < 0 || c_total <= 0 || c_off + c > c_total) return MC_EINVAL;
  int rc;
  if ((rc = check_gsrc(g))) return rc;
  if (g->kind != MC_GSRC_PLAIN && g->kind != MC_GSRC_PADFOLD) return MC_EUNSUPPORTED;     // (what a concat's consumer hands it)
  if (g->c8_total != 0 || g->hs != h || g->ws != w) return MC_EINVAL;
  if (dtype != MC_F32 && !mc_is16(dtype)) return MC_EUNSUPPORTED;
  const int C8 = (c + 7) / 8, c8t = (c_total + 7) / 8;
  dim3 gr(max(1, min(cdiv(h * w, 256), 1024)), C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_cat_grad_gather<T>, gr, dim3(256), 0, s, *g, c8t, c_off, c, C8, h, w, (T*)out);
  });
}

int mc_gsrc_sum(const mc_grad_src* g0, const mc_grad_src* g1, int32_t n, int32_t c, int32_t h, int32_t w,
                int32_t dtype, void* out, void* stream) {
  if (!g0 || !out || n <= 0 || c <= 0 || h <= 0 || w <= 0) return MC_EINVAL;
  int rc;
  if ((rc = check_gsrc(g0)) || (rc = check_gsrc(g1))) return rc;
  const int C8 = (c + 7) / 8;
  dim3 g(max(1, min(cdiv(h * w, 256 * 4), 1024)), C8, n);
  hipStream_t s = (hipStream_t)stream;
  return with_grad_type(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(k_gsrc_sum<T>, g, dim3(256), 0, s, gsrc_or_none(g0), gsrc_or_none(g1), C8, h, w, (T*)out);
  });
}

}  // extern "C"

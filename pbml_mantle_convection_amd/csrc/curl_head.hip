// Output heads on NCHW f32: velocity as the curl of the streamfunction (U-Net form with wall fix-up, FluidNet valid
// form), their adjoints, and torch.clip of the temperature channel.
#include "common.h"
#include "launch.h"

namespace {

// =================================================================================================
// curl head (Unet :2038-2068)
// =================================================================================================
// raw stencil values (before wall/corner fix-up) at interior-clamped positions
__device__ __forceinline__ float curl_u_raw(const float* a, int y, int x, int H, int W) {
  // u_in[y'][x'] = 0.5 (a[y'+2][x'+1] - a[y'][x'+1]), y' in [0,H-3], x' in [0,W-3]; replicate pad by 1
  int yc = min(max(y - 1, 0), H - 3), xc = min(max(x - 1, 0), W - 3);
  return 0.5f * (a[(size_t)(yc + 2) * W + xc + 1] - a[(size_t)yc * W + xc + 1]);
}
__device__ __forceinline__ float curl_v_raw(const float* a, int y, int x, int H, int W) {
  int yc = min(max(y - 1, 0), H - 3), xc = min(max(x - 1, 0), W - 3);
  return -0.5f * (a[(size_t)(yc + 1) * W + xc + 2] - a[(size_t)(yc + 1) * W + xc]);
}

__global__ void k_curl_fwd(const float* __restrict__ a_, int H, int W, int64_t abs_, float ab, float* __restrict__ u,
                           float* __restrict__ v) {
  const int n = blockIdx.y;
  const float* a = a_ + (size_t)n * abs_;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W; i += gridDim.x * blockDim.x) {
    int y = i / W, x = i % W;
    bool corner = (y == 0 || y == H - 1) && (x == 0 || x == W - 1);
    float uu, vv;
    if (x == 0) uu = -curl_u_raw(a, y, 1, H, W);
    else if (x == W - 1) uu = -curl_u_raw(a, y, W - 2, H, W);
    else uu = curl_u_raw(a, y, x, H, W);
    if (y == 0) vv = -curl_v_raw(a, 1, x, H, W);
    else if (y == H - 1) vv = -curl_v_raw(a, H - 2, x, H, W);
    else vv = curl_v_raw(a, y, x, H, W);
    u[(size_t)n * H * W + i] = corner ? 0.f : ab * uu;
    v[(size_t)n * H * W + i] = corner ? 0.f : ab * vv;
  }
}

// adjoint: fold the wall / replicate structure of (gu, gv) onto the interior stencil outputs,
// then apply the transposed stencils.
__global__ void k_curl_bwd_fold(const float* __restrict__ gu, const float* __restrict__ gv, int H, int W,
                                float* __restrict__ eu, float* __restrict__ ev) {
  // eu/ev: [n][H-2][W-2] effective gradients w.r.t. the stencil outputs u_in, v_in
  const int n = blockIdx.y;
  const float* gun = gu + (size_t)n * H * W;
  const float* gvn = gv + (size_t)n * H * W;
  const int Hi = H - 2, Wi = W - 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hi * Wi; i += gridDim.x * blockDim.x) {
    int yp = i / Wi, xp = i % Wi;
    // u: rows y with clamp(y-1)==yp : y = yp+1, plus y=0 if yp==0, y=H-1 if yp==H-3
    float su = 0.f, sv = 0.f;
    int ys[3], ny = 0;
    ys[ny++] = yp + 1;
    if (yp == 0) ys[ny++] = 0;
    if (yp == Hi - 1) ys[ny++] = H - 1;
    int xs[3], nx = 0;
    xs[nx++] = xp + 1;
    if (xp == 0) xs[nx++] = 0;
    if (xp == Wi - 1) xs[nx++] = W - 1;
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) {
        int y = ys[a], x = xs[b];
        bool corner = (y == 0 || y == H - 1) && (x == 0 || x == W - 1);
        if (corner) continue;
        // u: wall columns x==0 / W-1 take -u[:, 1] / -u[:, W-2], which are u_in[.., 0] / u_in[.., W-3]
        su += ((x == 0 || x == W - 1) ? -1.f : 1.f) * gun[(size_t)y * W + x];
        sv += ((y == 0 || y == H - 1) ? -1.f : 1.f) * gvn[(size_t)y * W + x];
      }
    eu[(size_t)n * Hi * Wi + i] = su;
    ev[(size_t)n * Hi * Wi + i] = sv;
  }
}

__global__ void k_curl_bwd_stencil(const float* __restrict__ eu, const float* __restrict__ ev, int H, int W, float ab,
                                   float* __restrict__ ga_, int64_t gabs) {
  const int n = blockIdx.y;
  const int Hi = H - 2, Wi = W - 2;
  const float* eun = eu + (size_t)n * Hi * Wi;
  const float* evn = ev + (size_t)n * Hi * Wi;
  float* ga = ga_ + (size_t)n * gabs;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < H * W; i += gridDim.x * blockDim.x) {
    int y = i / W, x = i % W;
    float acc = 0.f;
    // u_in[yp][xp] = 0.5 (a[yp+2][xp+1] - a[yp][xp+1])
    int xp = x - 1;
    if (xp >= 0 && xp < Wi) {
      if (y - 2 >= 0 && y - 2 < Hi) acc += 0.5f * eun[(size_t)(y - 2) * Wi + xp];
      if (y < Hi) acc -= 0.5f * eun[(size_t)y * Wi + xp];
    }
    // v_in[yp][xp] = -0.5 (a[yp+1][xp+2] - a[yp+1][xp])
    int yp = y - 1;
    if (yp >= 0 && yp < Hi) {
      if (x - 2 >= 0 && x - 2 < Wi) acc -= 0.5f * evn[(size_t)yp * Wi + x - 2];
      if (x < Wi) acc += 0.5f * evn[(size_t)yp * Wi + x];
    }
    ga[i] = ab * acc;
  }
}

// curl head of FluidNet (:1681-1697): the conv stack grew the field to (H+2) x (W+2), so the centred differences of the
// streamfunction land exactly on H x W -- no wall fix-up, no workspace.  One thread per output pixel, rows along x (coalesced).
__global__ void __launch_bounds__(256) k_curl_valid_fwd(const float* __restrict__ a_, int H, int W, int64_t abs_, float ab,
                                                        float* __restrict__ u, float* __restrict__ v) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y, n = blockIdx.z;
  if (x >= W || y >= H) return;
  const int Wa = W + 2;
  const float* a = a_ + (size_t)n * abs_;
  const float uu = 0.5f * (a[(size_t)(y + 2) * Wa + x + 1] - a[(size_t)y * Wa + x + 1]);
  const float vv = -0.5f * (a[(size_t)(y + 1) * Wa + x + 2] - a[(size_t)(y + 1) * Wa + x]);
  u[((size_t)n * H + y) * W + x] = ab * uu;
  v[((size_t)n * H + y) * W + x] = ab * vv;
}

// adjoint as a gather over the whole (H+2) x (W+2) plane: every pixel of ga is written (no memset), each by one thread from
// at most four terms in a fixed order (bit-reproducible: no atomics)
__global__ void __launch_bounds__(256) k_curl_valid_bwd(const float* __restrict__ gu_, const float* __restrict__ gv_, int H, int W,
                                                        float ab, float* __restrict__ ga_, int64_t gabs) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y * blockDim.y + threadIdx.y, n = blockIdx.z;
  if (c >= W + 2 || r >= H + 2) return;
  const float* gu = gu_ + (size_t)n * H * W;
  const float* gv = gv_ + (size_t)n * H * W;
  float acc = 0.f;
  // u[i][j] = 0.5 (a[i+2][j+1] - a[i][j+1]):  + gu[r-2][c-1], - gu[r][c-1]
  const int j = c - 1;
  if (j >= 0 && j < W) {
    if (r - 2 >= 0 && r - 2 < H) acc += gu[(size_t)(r - 2) * W + j];
    if (r < H) acc -= gu[(size_t)r * W + j];
  }
  // v[i][j] = -0.5 (a[i+1][j+2] - a[i+1][j]):  - gv[r-1][c-2], + gv[r-1][c]
  const int i = r - 1;
  if (i >= 0 && i < H) {
    if (c - 2 >= 0 && c - 2 < W) acc -= gv[(size_t)i * W + c - 2];
    if (c < W) acc += gv[(size_t)i * W + c];
  }
  ga_[(size_t)n * gabs + (size_t)r * (W + 2) + c] = ab * 0.5f * acc;
}

// =================================================================================================
// blurred streamfunction (NewFluidNet :1357-1361, FluidNet :1682-1686): B = 3 x 3 box mean of A = a_bound * a over the
// replicate-padded Hp x Wp plane, weight w = float(1) / float(9) on every tap; u, v are the heads above applied to B.  The
// mean is fused into the head, so neither B nor its gradient ever exists in memory.
// =================================================================================================
constexpr int BT_X = 64, BT_Y = 16;                 // output tile of one 64 x 4 block: every thread makes four rows
constexpr float BLUR_W = 1.0f / 9.0f;               // the f32 weight of the reference's filter

// Forward, both forms.  A centre (ye, xe) of the plane gives
//   u_in = 0.5 (B[ye+1][xe] - B[ye-1][xe]),  v_in = -0.5 (B[ye][xe+1] - B[ye][xe-1]);
// the middle row (column) of the two box sums is shared and cancels, so twelve taps remain per component.
// WALL (Unet / NewFluidNet form, output Hp x Wp): ye = clamp(y, 1, Hp-2), xe = clamp(x, 1, Wp-2) is the replicate pad of
// u_in / v_in, wall columns of u and wall rows of v change sign, corners are 0.  Otherwise (FluidNet form, output
// (Hp-2) x (Wp-2)): ye = y + 1, xe = x + 1.  The block stages the (BT_Y + 4) x (BT_X + 4) window around its centres with
// indices clamped to the plane: the clamp is the blur's replicate rule, and no read leaves the plane of item n.
template <bool WALL>
__global__ void __launch_bounds__(256) k_curl_blur_fwd(const float* __restrict__ a_, int Hp, int Wp, int64_t abs_, float ab,
                                                       float* __restrict__ u, float* __restrict__ v) {
  __shared__ float s[BT_Y + 4][BT_X + 4];
  const int n = blockIdx.z, tx0 = blockIdx.x * BT_X, ty0 = blockIdx.y * BT_Y;
  const int Ho = WALL ? Hp : Hp - 2, Wo = WALL ? Wp : Wp - 2;
  const int oy = (WALL ? min(max(ty0, 1), Hp - 2) : ty0 + 1) - 2, ox = (WALL ? min(max(tx0, 1), Wp - 2) : tx0 + 1) - 2;
  const float* a = a_ + (size_t)n * abs_;
  for (int r = threadIdx.y; r < BT_Y + 4; r += 4) {
    const float* row = a + (size_t)min(max(oy + r, 0), Hp - 1) * Wp;
    for (int c = threadIdx.x; c < BT_X + 4; c += 64) s[r][c] = row[min(max(ox + c, 0), Wp - 1)];
  }
  __syncthreads();
  const int x = tx0 + threadIdx.x;
  if (x >= Wo) return;
  const float k = ab * (0.5f * BLUR_W);
  const int lx = (WALL ? min(max(x, 1), Wp - 2) : x + 1) - ox;
  const bool wall_x = WALL && (x == 0 || x == Wp - 1);
#pragma unroll
  for (int j = 0; j < BT_Y / 4; ++j) {
    const int y = ty0 + threadIdx.y + 4 * j;
    if (y >= Ho) break;
    const int ly = (WALL ? min(max(y, 1), Hp - 2) : y + 1) - oy;
    const bool wall_y = WALL && (y == 0 || y == Hp - 1);
    float su[3], sv[3];
#pragma unroll
    for (int d = -1; d <= 1; ++d) {
      su[d + 1] = (s[ly + 2][lx + d] - s[ly - 2][lx + d]) + (s[ly + 1][lx + d] - s[ly - 1][lx + d]);
      sv[d + 1] = (s[ly + d][lx + 2] - s[ly + d][lx - 2]) + (s[ly + d][lx + 1] - s[ly + d][lx - 1]);
    }
    const float uu = k * ((su[0] + su[1]) + su[2]), vv = -(k * ((sv[0] + sv[1]) + sv[2]));
    const bool corner = wall_x && wall_y;
    const size_t o = ((size_t)n * Ho + y) * Wo + x;
    u[o] = corner ? 0.f : (wall_x ? -uu : uu);
    v[o] = corner ? 0.f : (wall_y ? -vv : vv);
  }
}

// Adjoint, both forms: eu, ev [n][Hp-2][Wp-2] are the gradients w.r.t. u_in, v_in (k_curl_bwd_fold's output, or gu, gv
// themselves in the FluidNet form).  The stencil adjoint
//   gB[r][c] = ((eu[r-2][c-1] - eu[r][c-1]) - ev[r-1][c-2]) + ev[r-1][c]     (terms outside eu / ev are 0)
// is formed while the block stages its (BT_Y + 2) x (BT_X + 2) window, again at indices clamped to the plane.  The clamped
// box mean is a symmetric matrix (rows 0 and Hp-1 count themselves twice), so its transpose is the same clamped 3 x 3 sum:
//   ga[r][c] = a_bound 0.5 w sum_{dr, dc} gB[clamp(r+dr)][clamp(c+dc)].
// Every pixel of the plane is written once by one thread in a fixed order: no memset, no atomics.
__device__ __forceinline__ float curl_gB(const float* __restrict__ eu, const float* __restrict__ ev, int r, int c, int Hi, int Wi) {
  float acc = 0.f;
  const int j = c - 1, i = r - 1;
  if (j >= 0 && j < Wi) {
    if (r - 2 >= 0 && r - 2 < Hi) acc += eu[(size_t)(r - 2) * Wi + j];
    if (r < Hi) acc -= eu[(size_t)r * Wi + j];
  }
  if (i >= 0 && i < Hi) {
    if (c - 2 >= 0 && c - 2 < Wi) acc -= ev[(size_t)i * Wi + c - 2];
    if (c < Wi) acc += ev[(size_t)i * Wi + c];
  }
  return acc;
}

__global__ void __launch_bounds__(256) k_curl_blur_bwd(const float* __restrict__ eu_, const float* __restrict__ ev_, int Hp, int Wp,
                                                       float ab, float* __restrict__ ga_, int64_t gabs) {
  __shared__ float s[BT_Y + 2][BT_X + 2];
  const int n = blockIdx.z, tx0 = blockIdx.x * BT_X, ty0 = blockIdx.y * BT_Y;
  const int Hi = Hp - 2, Wi = Wp - 2;
  const float* eu = eu_ + (size_t)n * Hi * Wi;
  const float* ev = ev_ + (size_t)n * Hi * Wi;
  for (int r = threadIdx.y; r < BT_Y + 2; r += 4) {
    const int pr = min(max(ty0 - 1 + r, 0), Hp - 1);
    for (int c = threadIdx.x; c < BT_X + 2; c += 64) s[r][c] = curl_gB(eu, ev, pr, min(max(tx0 - 1 + c, 0), Wp - 1), Hi, Wi);
  }
  __syncthreads();
  const int c = tx0 + threadIdx.x;
  if (c >= Wp) return;
  const float k = ab * (0.5f * BLUR_W);
  const int lx = threadIdx.x + 1;
  float* ga = ga_ + (size_t)n * gabs;
#pragma unroll
  for (int j = 0; j < BT_Y / 4; ++j) {
    const int ly = threadIdx.y + 4 * j + 1, r = ty0 + ly - 1;
    if (r >= Hp) break;
    float t[3];
#pragma unroll
    for (int d = -1; d <= 1; ++d) t[d + 1] = (s[ly + d][lx - 1] + s[ly + d][lx]) + s[ly + d][lx + 1];
    ga[(size_t)r * Wp + c] = k * ((t[0] + t[1]) + t[2]);
  }
}

__global__ void k_clip_fwd(const float* __restrict__ t, int hw, int64_t bs, float lo, float hi, float* __restrict__ o) {
  const int n = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x)
    o[(size_t)n * hw + i] = fminf(fmaxf(t[(size_t)n * bs + i], lo), hi);
}
// torch.clip passes the gradient where lo <= x <= hi
__global__ void k_clip_bwd(const float* __restrict__ go, const float* __restrict__ t, int hw, int64_t bs, int64_t gbs, float lo,
                           float hi, float* __restrict__ gi) {
  const int n = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
    float x = t[(size_t)n * bs + i];
    gi[(size_t)n * gbs + i] = (x >= lo && x <= hi) ? go[(size_t)n * hw + i] : 0.f;
  }
}

}  // namespace

extern "C" {

int mc_curl_head_fwd(const float* a, const float* t_in, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride,
                     float a_bound, float t_lo, float t_hi, float* u, float* v, float* t_out, void* stream) {
  if (!a || !u || !v || n <= 0 || h < 3 || w < 3 || ((t_in == nullptr) != (t_out == nullptr))) return MC_EINVAL;
  dim3 g(min(cdiv(h * w, 256), 4096), n);
  hipLaunchKernelGGL(k_curl_fwd, g, dim3(256), 0, (hipStream_t)stream, a, h, w, in_batch_stride, a_bound, u, v);
  if (t_in) hipLaunchKernelGGL(k_clip_fwd, g, dim3(256), 0, (hipStream_t)stream, t_in, h * w, in_batch_stride, t_lo, t_hi, t_out);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_curl_head_bwd(const float* gu, const float* gv, const float* gt_out, const float* t_in, int32_t n, int32_t h,
                     int32_t w, float a_bound, float t_lo, float t_hi, float* ga, float* gt_in, int64_t g_batch_stride,
                     int64_t in_batch_stride, float* ws, void* stream) {
  if (!gu || !gv || !ga || !ws || n <= 0 || h < 3 || w < 3) return MC_EINVAL;
  if (gt_in && (!gt_out || !t_in)) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* eu = ws;
  float* ev = ws + (size_t)n * (h - 2) * (w - 2);
  dim3 g1(min(cdiv((h - 2) * (w - 2), 256), 4096), n);
  hipLaunchKernelGGL(k_curl_bwd_fold, g1, dim3(256), 0, s, gu, gv, h, w, eu, ev);
  dim3 g2(min(cdiv(h * w, 256), 4096), n);
  hipLaunchKernelGGL(k_curl_bwd_stencil, g2, dim3(256), 0, s, eu, ev, h, w, a_bound, ga, g_batch_stride);
  if (gt_in) hipLaunchKernelGGL(k_clip_bwd, g2, dim3(256), 0, s, gt_out, t_in, h * w, in_batch_stride, g_batch_stride, t_lo, t_hi, gt_in);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_curl_valid_fwd(const float* a, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride, float a_bound, float* u,
                      float* v, void* stream) {
  if (!a || !u || !v || n <= 0 || n > 65535 || h <= 0 || w <= 0 || in_batch_stride < (int64_t)(h + 2) * (w + 2)) return MC_EINVAL;
  dim3 g(cdiv(w, 64), cdiv(h, 4), n);
  hipLaunchKernelGGL(k_curl_valid_fwd, g, dim3(64, 4), 0, (hipStream_t)stream, a, h, w, in_batch_stride, a_bound, u, v);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_curl_valid_bwd(const float* gu, const float* gv, int32_t n, int32_t h, int32_t w, float a_bound, float* ga,
                      int64_t g_batch_stride, void* stream) {
  if (!gu || !gv || !ga || n <= 0 || n > 65535 || h <= 0 || w <= 0 || g_batch_stride < (int64_t)(h + 2) * (w + 2)) return MC_EINVAL;
  dim3 g(cdiv(w + 2, 64), cdiv(h + 2, 4), n);
  hipLaunchKernelGGL(k_curl_valid_bwd, g, dim3(64, 4), 0, (hipStream_t)stream, gu, gv, h, w, a_bound, ga, g_batch_stride);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

// ---- the same four heads with the 3 x 3 box mean of the streamfunction inside (same arguments, same workspace) ----
int mc_curl_blur_head_fwd(const float* a, const float* t_in, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride,
                          float a_bound, float t_lo, float t_hi, float* u, float* v, float* t_out, void* stream) {
  if (!a || !u || !v || n <= 0 || n > 65535 || h < 3 || w < 3 || ((t_in == nullptr) != (t_out == nullptr))) return MC_EINVAL;
  dim3 g(cdiv(w, BT_X), cdiv(h, BT_Y), n);
  hipLaunchKernelGGL(k_curl_blur_fwd<true>, g, dim3(64, 4), 0, (hipStream_t)stream, a, h, w, in_batch_stride, a_bound, u, v);
  if (t_in) {
    dim3 gc(min(cdiv(h * w, 256), 4096), n);
    hipLaunchKernelGGL(k_clip_fwd, gc, dim3(256), 0, (hipStream_t)stream, t_in, h * w, in_batch_stride, t_lo, t_hi, t_out);
  }
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_curl_blur_head_bwd(const float* gu, const float* gv, const float* gt_out, const float* t_in, int32_t n, int32_t h,
                          int32_t w, float a_bound, float t_lo, float t_hi, float* ga, float* gt_in, int64_t g_batch_stride,
                          int64_t in_batch_stride, float* ws, void* stream) {
  if (!gu || !gv || !ga || !ws || n <= 0 || n > 65535 || h < 3 || w < 3) return MC_EINVAL;
  if (gt_in && (!gt_out || !t_in)) return MC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  float* eu = ws;
  float* ev = ws + (size_t)n * (h - 2) * (w - 2);
  dim3 g1(min(cdiv((h - 2) * (w - 2), 256), 4096), n);
  hipLaunchKernelGGL(k_curl_bwd_fold, g1, dim3(256), 0, s, gu, gv, h, w, eu, ev);
  dim3 g2(cdiv(w, BT_X), cdiv(h, BT_Y), n);
  hipLaunchKernelGGL(k_curl_blur_bwd, g2, dim3(64, 4), 0, s, eu, ev, h, w, a_bound, ga, g_batch_stride);
  if (gt_in) {
    dim3 gc(min(cdiv(h * w, 256), 4096), n);
    hipLaunchKernelGGL(k_clip_bwd, gc, dim3(256), 0, s, gt_out, t_in, h * w, in_batch_stride, g_batch_stride, t_lo, t_hi, gt_in);
  }
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_curl_blur_valid_fwd(const float* a, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride, float a_bound, float* u,
                           float* v, void* stream) {
  if (!a || !u || !v || n <= 0 || n > 65535 || h <= 0 || w <= 0 || in_batch_stride < (int64_t)(h + 2) * (w + 2)) return MC_EINVAL;
  dim3 g(cdiv(w, BT_X), cdiv(h, BT_Y), n);
  hipLaunchKernelGGL(k_curl_blur_fwd<false>, g, dim3(64, 4), 0, (hipStream_t)stream, a, h + 2, w + 2, in_batch_stride, a_bound, u, v);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

int mc_curl_blur_valid_bwd(const float* gu, const float* gv, int32_t n, int32_t h, int32_t w, float a_bound, float* ga,
                           int64_t g_batch_stride, void* stream) {
  if (!gu || !gv || !ga || n <= 0 || n > 65535 || h <= 0 || w <= 0 || g_batch_stride < (int64_t)(h + 2) * (w + 2)) return MC_EINVAL;
  dim3 g(cdiv(w + 2, BT_X), cdiv(h + 2, BT_Y), n);
  hipLaunchKernelGGL(k_curl_blur_bwd, g, dim3(64, 4), 0, (hipStream_t)stream, gu, gv, h + 2, w + 2, a_bound, ga, g_batch_stride);
  MC_CHECK_LAUNCH();
  return MC_OK;
}

}  // extern "C"

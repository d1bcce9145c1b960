// Host-side launch helpers shared by the streaming-kernel units (layout, groupnorm, bicubic, curl_head): environment
// knobs, grid shapes, the dtype -> element type maps, gradient-source descriptor checks, the frame shape of the padding folds.
#pragma once
#include <stdlib.h>
#include "common.h"

static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

inline dim3 grid1(size_t total, int block = 256, int cap = 8192) {
  size_t g = (total + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return dim3((unsigned)g);
}
inline dim3 grid3(int per_plane, int c8, int n, int block = 256, int capx = 64) {
  int gx = (per_plane + block - 1) / block;
  if (gx > capx) gx = capx;
  if (gx < 1) gx = 1;
  return dim3(gx, c8, n);
}

// The three maps from the `dtype` of the C ABI to the element types a kernel is instantiated with.  Each helper calls f,
// which launches, with one TypeTag per type (in f: `using T = typename decltype(t)::type;`) and returns what the launch
// left (MC_OK or its HIP error), or MC_EUNSUPPORTED without calling f for a dtype outside the map.  A launch that exists for
// fewer types than a map lists keeps its own ladder: the helpers instantiate f for every type of their map.
template <typename T> struct TypeTag { using type = T; };
// storage type of activations: MC_F32 -> float, MC_BF16 -> bf16_t, MC_MIX16 -> f16_t
template <typename F> static int with_storage_type(int dtype, F&& f) {
  if (dtype == MC_F32) f(TypeTag<float>{});
  else if (dtype == MC_BF16) f(TypeTag<bf16_t>{});
  else if (dtype == MC_MIX16) f(TypeTag<f16_t>{});
  else return MC_EUNSUPPORTED;
  MC_CHECK_LAUNCH();
  return MC_OK;
}
// gradient type: MC_F32 -> float, MC_BF16 and MC_MIX16 -> bf16_t
template <typename F> static int with_grad_type(int dtype, F&& f) {
  if (dtype == MC_F32) f(TypeTag<float>{});
  else if (mc_is16(dtype)) f(TypeTag<bf16_t>{});
  else return MC_EUNSUPPORTED;
  MC_CHECK_LAUNCH();
  return MC_OK;
}
// gradient type T with the storage type TY of y: (float, float), (bf16_t, bf16_t), MC_MIX16 -> (bf16_t, f16_t)
template <typename F> static int with_grad_y_types(int dtype, F&& f) {
  if (dtype == MC_F32) f(TypeTag<float>{}, TypeTag<float>{});
  else if (dtype == MC_BF16) f(TypeTag<bf16_t>{}, TypeTag<bf16_t>{});
  else if (dtype == MC_MIX16) f(TypeTag<bf16_t>{}, TypeTag<f16_t>{});
  else return MC_EUNSUPPORTED;
  MC_CHECK_LAUNCH();
  return MC_OK;
}

static int check_gsrc(const mc_grad_src* g) {
  if (!g) return MC_OK;
  if (g->kind == MC_GSRC_NONE) return MC_OK;
  if (!g->ptr || g->hs <= 0 || g->ws <= 0) return MC_EINVAL;
  if (g->kind < MC_GSRC_NONE || g->kind > MC_GSRC_PLAIN_POOL) return MC_EINVAL;
  if ((g->kind == MC_GSRC_PADFOLD_POOL || g->kind == MC_GSRC_PLAIN_POOL) && g->pool < 1) return MC_EINVAL;
  if ((g->kind == MC_GSRC_PADFOLD || g->kind == MC_GSRC_PADFOLD_POOL) && (g->pad < 0 || g->pad > 2)) return MC_EUNSUPPORTED;
  if (g->c8_total < 0 || g->cb_off < 0 || (g->c8_total > 0 && g->cb_off >= g->c8_total)) return MC_EINVAL;
  return MC_OK;
}
static mc_grad_src gsrc_or_none(const mc_grad_src* g) {
  mc_grad_src z;
  z.ptr = nullptr; z.kind = MC_GSRC_NONE; z.pad = 0; z.pad_mode = 0; z.pool = 1; z.hs = 0; z.ws = 0; z.c8_total = 0; z.cb_off = 0;
  return g ? *g : z;
}

// band + side pixels of the frame a padding fold visits (`all`: the image is smaller than two frames, every pixel)
static void fold_shape(int hs, int ws, int pad, int& all, int& total) {
  const int t = pad + 1;
  all = (hs < 2 * t || ws < 2 * t) ? 1 : 0;
  total = all ? hs * ws : 2 * t * ws + (hs - 2 * t) * 2 * t;
}

/*
 * mantle_hip.h — C ABI of libmantle_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the Stokes-surrogate training hot path of
 * agsiddhant/PBML_Mantle_Convection.  The reference has no FFI / operator registry: its
 * boundary is the Python surface, whose numeric back end is PyTorch ATen.
 * Every entry point below replaces the ATen call sequence of one reference call site
 * (cited per function, paths relative to the reference tree).  Host code (Python, ctypes)
 * mirrors the reference's module/trainer API on top of these.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.  `stream` is a hipStream_t
 *    passed as void*.  All calls are asynchronous on `stream`, stateless and re-entrant.
 *  - The caller owns every buffer (including workspaces); the library never allocates,
 *    frees or retains device memory.
 *  - Return 0 on success; MC_E* (negative) for argument/shape/unsupported errors;
 *    positive values are hipError_t codes from the launch.  Nothing throws or aborts.
 *  - Activations use the CB8 layout: [N][C8][H][W][8] with C8 = ceil(C/8) channel blocks,
 *    element type f32 (MC_F32), bf16 (MC_BF16) or f16 forward / bf16 gradients (MC_MIX16).  Padded channels hold zeros.
 *    Network inputs/outputs and loss fields are plain NCHW / NHW f32.
 *  - Parameters are read in the REFERENCE's layout (unique mirrored-filter bank
 *    [U][C_in][k][k] f32, bias [C_out] f32; symmetric_layers_torch.py:96-107).
 */
#ifndef MANTLE_HIP_H
#define MANTLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_OK 0
#define MC_EINVAL (-1)
#define MC_EUNSUPPORTED (-2)
#define MC_EWORKSPACE (-3)

/* MC_MIX16 (the trainer's "mixed" precision): every tensor of the FORWARD pass (packed input, filter banks of the forward
 * convolutions, raw conv outputs, activations, pooled / upsampled tensors) is IEEE f16, every GRADIENT tensor (dY, dA,
 * padded-domain input gradients, their filter banks) is bf16; MFMA arithmetic with f32 accumulation either way.  An entry
 * point that takes `dtype` reads / writes each of its operands in the type of that operand's role: forward-only calls
 * (mc_pack_nchw, mc_gn_act_fwd, mc_bicubic_fwd ...) move f16, gradient-only calls (mc_fold_padded, mc_bicubic_bwd ...) move
 * bf16, the GroupNorm-backward and filter-gradient calls read y / x as f16 and gradients as bf16. */
enum { MC_F32 = 0, MC_BF16 = 1, MC_MIX16 = 2 };
enum { MC_PAD_ZEROS = 0, MC_PAD_REPLICATE = 1, MC_PAD_REFLECT = 2 };
enum { MC_ACT_NONE = 0, MC_ACT_GELU = 1, MC_ACT_RELU = 2, MC_ACT_SILU = 3, MC_ACT_TANH = 4,
       MC_ACT_SELU = 5, MC_ACT_ELU = 6 };
/* what follows the convolution inside one reference layer */
enum { MC_POST_NONE = 0,   /* plain nn.Conv2d (Unet conv[-1], ConvAE final conv)          */
       MC_POST_ACT = 1,    /* conv -> act (Unet conv[-2])                                  */
       MC_POST_GN_ACT = 2  /* conv -> GroupNorm -> act (FluidLayer; Unet conv[-3] + gn[0]) */ };
/* where the gradient w.r.t. an activated tensor comes from (backward) */
enum { MC_GSRC_NONE = 0,
       MC_GSRC_PLAIN = 1,      /* CB8 tensor of the same H x W                                         */
       MC_GSRC_PADFOLD = 2,    /* dgrad output on the padded domain (H+2p)x(W+2p) whose halo has been      */
                               /* folded onto the interior by mc_fold_padded: read at offset (p, p)    */
       MC_GSRC_PADFOLD_POOL = 3, /* same, through the adjoint of AvgPool(f): value/f^2 at (y/f, x/f)  */
       MC_GSRC_PLAIN_POOL = 4  /* CB8 tensor of size hs x ws through the adjoint of AvgPool(f)        */ };

typedef struct {
  int32_t n;          /* batch                                                       */
  int32_t h, w;       /* INPUT spatial size                                          */
  int32_t c_in0;      /* channels of source 0                                        */
  int32_t c_in1;      /* channels of source 1 (torch.cat on dim 1) or 0              */
  int32_t c_out;
  int32_t k;          /* square kernel, 3 or 5                                       */
  int32_t pad;        /* per side; output is (h + 2 pad - k + 1) x (w + 2 pad - k + 1) */
  int32_t pad_mode;   /* MC_PAD_*                                                    */
  int32_t dtype;      /* MC_F32 | MC_BF16 | MC_MIX16 : element type of x0, x1, y (MC_MIX16: f16; the input-gradient
                         convolution of such a layer is described with MC_BF16)       */
  int32_t sym_h;      /* number of x-mirrored filters (SymmetricConv2d symmetry['h']), 0 = plain Conv2d */
  int32_t c_out_split;/* dgrad only: first c_out_split output channels go to y0, the rest to y1 (0 = all to y0) */
  int32_t out_f32;    /* 16-bit dtypes only: 1 = write y0 as f32 CB8 (the network's last conv: u, v, p, T are not
                         quantised); requires c_out <= 16 and no c_out_split */
  int32_t sym_v;      /* number of y-mirrored filters (symmetry['v']) and of filters mirrored about both axes (symmetry['hv'],  */
  int32_t sym_hv;     /* quadruples: x-, y- and xy-flips): output channels [U, c_out) in the reference's torch.cat order, */
                      /* U = c_out - sym_h/2 - sym_v/2 - 3 sym_hv/4 unique filters (symmetric_layers_torch.py:118-136)   */
} mc_conv_desc;

typedef struct {
  const void* ptr;    /* CB8 tensor, element type = desc dtype                        */
  int32_t kind;       /* MC_GSRC_*                                                    */
  int32_t pad;        /* p of the conv that produced the padded-domain gradient       */
  int32_t pad_mode;   /* MC_PAD_* of that conv                                        */
  int32_t pool;       /* f for MC_GSRC_PADFOLD_POOL                                   */
  int32_t hs, ws;     /* unpadded spatial size of the tensor `ptr` is the gradient of */
  int32_t c8_total;   /* > 0: `ptr` holds c8_total channel blocks per sample and this source is   */
  int32_t cb_off;     /* the slice starting at block cb_off (gradient of one torch.cat operand)   */
} mc_grad_src;

/* "Normalise on load": a consumer of a raw conv output y applies act(scale * y + shift) — GroupNorm's affine map folded
 * with its statistics, then the activation (FluidLayer.forward, pytorch_networks_convae.py:790-799) — while it stages its
 * input tile, so the activated tensor never crosses HBM.  coef tables: [n][ceil(c/8)*8][4] f32 = (scale, shift, mean,
 * rstd) per (sample, channel) from mc_gn_finalize_coef; NULL = no affine map.  act = MC_ACT_NONE with a NULL table
 * means the source is used as it is (network input, pooled / upsampled tensors). */
typedef struct {
  const float* coef0; /* source 0 */
  const float* coef1; /* source 1 (second torch.cat operand) */
  int32_t act0, act1; /* MC_ACT_* */
} mc_conv_prologue;

/* Input-gradient epilogue: the launch computes dA (gradient w.r.t. the ACTIVATED tensor a = act(GN(y))) on the padded
 * domain; with an epilogue it stores dz = dA * act'(z), z = scale*y + shift, instead and emits the per-tile partial
 * sums (sum dz, sum dz * yhat) per channel that GroupNorm's backward needs — the separate reduction pass over (dA, y)
 * disappears.  With reflect / replicate padding the pixels within pad+1 of the border still await the padding adjoint:
 * they are stored as raw dA and finished (fold + dz + their partial sums) by mc_fold_padded_dz. */
typedef struct {
  const void* y;      /* raw conv output of the layer that produced the tensor: CB8 [n][c8][hs][ws], dtype of the desc */
  const float* coef;  /* its (scale, shift, mean, rstd) table, or NULL for an activation-only layer */
  int32_t act;        /* MC_ACT_* */
  int32_t pad;        /* p of the forward conv: the interior starts at (p, p) of the padded-domain output */
  int32_t pad_mode;   /* MC_PAD_* of the forward conv */
  int32_t hs, ws;     /* interior (unpadded) size */
  float* partials;    /* [n][part_stride][c8*8][2] f32; this launch fills slots 0 .. mc_conv_tiles(desc) - 1 of a sample */
  int32_t part_stride;/* slots per sample (>= tiles; the slots behind the tiles are mc_fold_padded_dz's) */
  int32_t y_f16;      /* 1: y is f16 -- the layer belongs to an MC_MIX16 network (the launch itself is MC_BF16); else 0 */
} mc_conv_epilogue;

int mc_version(void);
const char* mc_strerror(int code);

/* ---- boundary layout conversion ---------------------------------------------------------- */
/* NCHW f32 -> CB8 with optional W padding (Unet.forward's F.pad(inputs,(3,3,0,0),mode=r_p),
 * pytorch_networks_convae.py:1991).  out is [n][ceil(c/8)][h][w + 2 pad_w][8]. */
/* x holds src_c >= c channels per sample (only the first c are taken: get_loss feeds the net the
 * first ten of gVTp's channels, multigpu.py:234-248); chan_scale (nullable, [c]) multiplies each
 * channel on the way in (xc/4, yc/4, dt/roll_forward). */
int mc_pack_nchw(const float* x, int32_t n, int32_t c, int32_t src_c, int32_t h, int32_t w, int32_t pad_w,
                 int32_t pad_mode, const float* chan_scale, int32_t dtype, void* out, void* stream);
/* CB8 -> NCHW f32, optionally subtracting a per-(n,c) mean and cropping crop_w columns on
 * both sides ((y - mean(y))[..., 3:-3], pytorch_networks_convae.py:2024).  mean may be NULL. */
int mc_unpack_nchw(const void* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t crop_w,
                   const float* mean_nc, int32_t dtype, float* out, void* stream);
/* adjoint of mc_unpack_nchw: g NCHW f32 [n][c][h][w - 2 crop_w] -> CB8 [n][c8][h][w][8],
 * zero in the cropped columns, minus mean_nc (the adjoint of the mean subtraction) if given. */
int mc_pack_grad_nchw(const float* g, int32_t n, int32_t c, int32_t h, int32_t w, int32_t crop_w,
                      const float* mean_nc, int32_t dtype, void* out, void* stream);
/* per-(n,c) sums of an NCHW f32 tensor, scaled: out[n*c] = scale * sum_hw x. */
int mc_sum_hw(const float* x, int32_t nc, int32_t hw, float scale, float* out, void* stream);

/* ---- convolution (SymmetricConv2d.forward symmetric_layers_torch.py:113-138 +
 *      nn.Conv2d._conv_forward: F.pad(mode) + F.conv2d; FluidLayer :764-786, Unet heads :1933-1979) */
/* Bytes of the packed filter bank mc_pack_weights writes for this descriptor / direction. */
size_t mc_packed_weight_bytes(const mc_conv_desc* d, int32_t dgrad);
/* Expand the unique mirrored-filter bank (never materialised in the reference layout: the
 * x-flipped copies are generated while packing) into the kernel-side bank.  dgrad != 0 packs
 * the transposed, 180-degree-rotated bank used by mc_conv2d for the input gradient. */
int mc_pack_weights(const mc_conv_desc* d, const float* w_unique, int32_t dgrad, void* packed,
                    void* stream);
/* Symbol-style name of the kernel instantiation mc_conv2d launches for this descriptor (static string;
 * lets a profiler trace be matched to a descriptor). */
const char* mc_conv_kernel_name(const mc_conv_desc* d);
/* Number of spatial tiles per image the conv kernel uses for this descriptor (sizes stat partials). */
int32_t mc_conv_tiles(const mc_conv_desc* d);
/* y = conv(pad(cat(x0,x1))) + bias.  y0 (and y1 when c_out_split) are CB8 outputs.
 * stat_partials (nullable): [n][tiles][c_out8*8][2] f32 per-tile (sum, sum of squares) of y,
 * taken from the f32 accumulators — the first half of GroupNorm (FluidLayer :788). */
int mc_conv2d(const mc_conv_desc* d, const void* x0, const void* x1, const void* packed_w,
              const float* bias, void* y0, void* y1, float* stat_partials, void* stream);
/* The same convolution with the producer's GroupNorm + activation applied to its sources on load (pro, nullable) and,
 * for an input-gradient launch, the GroupNorm-backward reduction fused into the epilogue (epi, nullable; needs a
 * single-source, unsplit output).  FluidLayer.forward :790-799 and its autograd backward. */
int mc_conv2d_fused(const mc_conv_desc* d, const void* x0, const void* x1, const mc_conv_prologue* pro,
                    const void* packed_w, const float* bias, void* y0, void* y1, float* stat_partials,
                    const mc_conv_epilogue* epi, void* stream);
/* Name of the instantiation mc_conv2d_fused launches for (d, pro, epi): the family name of mc_conv_kernel_name with, inside the
 * brackets, ",norm" (prologue) or ",dz" (epilogue), ",act" where the row-reuse kernel takes its generic-activation build (not
 * the GELU-only one), ",h16" when the launch reads f16, ",dzm" for the row-reuse epilogue on the MFMA waves.  Host only:
 * launches nothing and needs no device; pro / epi are validated as by the launch ("unsupported" where it would fail; their
 * pointers are not dereferenced).  Both NULL, or a prologue with nothing to do: the name mc_conv_kernel_name returns. */
const char* mc_conv_fused_kernel_name(const mc_conv_desc* d, const mc_conv_prologue* pro, const mc_conv_epilogue* epi);
/* Filter/bias gradient. partials: workspace of mc_wgrad_partial_bytes(d); the second call
 * reduces it deterministically, folds mirrored filters back onto the unique bank
 * (dW_unique[i] += flip_x(dW_full[U+i])) and ACCUMULATES into dw_unique / dbias. */
size_t mc_wgrad_partial_bytes(const mc_conv_desc* d);
/* One byte past the highest address a forward launch described by `d` reads through packed_w (the kernels' own indexing,
 * restated on the host).  For every layer: mc_conv_bank_read_extent(d) <= mc_packed_weight_bytes(d, 0), and for its
 * input-gradient launch dd: mc_conv_bank_read_extent(dd) <= mc_packed_weight_bytes(d, 1) (tests/test_abi_and_host.py). */
size_t mc_conv_bank_read_extent(const mc_conv_desc* d);
int mc_conv2d_wgrad(const mc_conv_desc* d, const void* x0, const void* x1, const void* dy,
                    void* partials, void* stream);
int mc_conv2d_wgrad_finalize(const mc_conv_desc* d, const void* partials, float* dw_unique,
                             float* dbias, void* stream);
/* mc_conv2d_wgrad with x0 / x1 given as RAW conv outputs: the activation is re-applied on load (pro as in mc_conv2d_fused). */
int mc_conv2d_wgrad_fused(const mc_conv_desc* d, const void* x0, const void* x1, const mc_conv_prologue* pro,
                          const void* dy, void* partials, void* stream);
/* mc_conv2d_wgrad for a conv -> GroupNorm -> act layer whose dz = dA act'(z) exists (mc_conv2d_fused's epilogue +
 * mc_fold_padded_dz) but whose dy does not: the launch forms dy = cA dz + (cB (y - mean) + cC) -- the value mc_gn_bwd_apply_dz
 * writes, bit for bit -- while it stages its tiles, accumulates the filter gradient of that dy and stores dy (bf16 CB8
 * [n][ceil(c_out/8)][ho][wo][8]) for the input-gradient launch that follows.  dz: MC_GSRC_PADFOLD or MC_GSRC_PLAIN of the
 * layer's output shape; y: the layer's raw conv output (f16); dz_coef: [n][ceil(c_out/8)*8][4] f32 = (cA, cB, cC, mean) from
 * mc_gn_act_bwd_finalize_dz / _n_dz, zeros in padded channels.  partials and mc_conv2d_wgrad_finalize as for mc_conv2d_wgrad
 * (the same slabs).  MC_EUNSUPPORTED unless dtype == MC_MIX16, the padded input channels fill at most 16 and c_out <= 16
 * (each dy tile is then staged by exactly one work-group), and dz has the layer's output shape. */
int mc_conv2d_wgrad_dz(const mc_conv_desc* d, const void* x0, const void* x1, const mc_grad_src* dz, const void* y,
                       const float* dz_coef, void* dy, void* partials, void* stream);
/* Batched forms (one launch for many layers; per-layer tables are plain host arrays of length n):
 * the per-step bank packing and the filter-gradient combine are tiny per layer and latency-bound when
 * launched one layer at a time. */
int mc_pack_weights_batched(const mc_conv_desc* descs, const float* const* w_unique, const int32_t* dgrad,
                            void* const* packed, int32_t n, void* stream);
int mc_conv2d_wgrad_finalize_batched(const mc_conv_desc* descs, const void* const* partials, float* const* dw_unique,
                                     float* const* dbias, int32_t n, void* stream);

/* Adjoint of F.pad(mode) on a padded-domain gradient (output of mc_conv2d in input-gradient mode):
 * adds the halo of buf [n][c8][hs+2p][ws+2p][8] onto the interior positions it was padded from
 * (reflect: mirror about the edge pixel; replicate: onto the edge pixel; zeros: nothing). In place;
 * touches only the O(p (H+W)) border pixels. */
int mc_fold_padded(void* buf, int32_t n, int32_t c, int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode,
                   int32_t dtype, void* stream);
/* The same for the two input-gradient outputs of a convolution over concatenated sources (same hs x ws, c0 and c1 channels)
 * in one launch; buf1 NULL = one buffer. */
int mc_fold_padded2(void* buf0, int32_t c0, void* buf1, int32_t c1, int32_t n, int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode,
                    int32_t dtype, void* stream);
/* Companion of mc_conv2d_fused's epilogue for reflect / replicate padding: folds the halo onto the frame pixels (within
 * pad+1 of the border) like mc_fold_padded, then turns them into dz = dA * act'(z) in place and writes their partial sums
 * into `partials` [n][mc_fold_blocks()][c8*8][2] (the caller passes the slots behind the conv tiles' of the same table). */
int32_t mc_fold_blocks(int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode);
int mc_fold_padded_dz(void* buf, int32_t n, int32_t c, int32_t hs, int32_t ws, int32_t pad, int32_t pad_mode,
                      int32_t dtype, const void* y, const float* coef, int32_t act, float* partials,
                      int32_t part_stride_blocks, int32_t part_first_block, void* stream);

/* ---- GroupNorm + activation (FluidLayer :788-799; Unet :2016-2021) ------------------------ */
/* Per-tile (sum, sum of squares) partials [n][tiles][ceil(c/8)*8][2] of an existing CB8 tensor, for layers whose output is
 * assembled from several convolutions (BoundaryLearnedConvolution2D) and cannot take them from one conv epilogue. */
int mc_gn_partials(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, int32_t tiles, float* part,
                   void* stream);
/* (mean, rstd) per (n, group) from conv stat partials; eps 1e-5, biased variance.  Also emits
 * per-(n,c) means of y when chan_mean != NULL (Unet's spatial zero-mean, :2024). */
int mc_gn_finalize(const float* stat_partials, int32_t n, int32_t tiles, int32_t c, int32_t groups,
                   int32_t hw, float eps, float* stats_ng2, float* chan_mean, void* stream);
/* mc_gn_finalize + the (scale, shift, mean, rstd) table [n][ceil(c/8)*8][4] that consumers of the raw conv output read
 * ("normalise on load"): scale = rstd * gamma, shift = beta - mean * rstd * gamma. */
int mc_gn_finalize_coef(const float* stat_partials, int32_t n, int32_t tiles, int32_t c, int32_t groups, int32_t hw,
                        float eps, const float* gamma, const float* beta, float* stats_ng2, float* coef4, void* stream);

/* a = act(GN(y));  post = MC_POST_*.  pool > 1 additionally writes AvgPool2d(pool)(a) into
 * pooled (Unet :2002, ConvAE :1051).  y, a, pooled are CB8 of `dtype`.  a may be NULL when pool > 1: only the pooled
 * tensor is materialised (the full-resolution consumers normalise y on load). */
int mc_gn_act_fwd(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                  const float* stats_ng2, const float* gamma, const float* beta, int32_t post,
                  int32_t act, int32_t pool, int32_t dtype, void* a, void* pooled, void* stream);
/* Small layers: mc_gn_finalize + mc_gn_act_fwd in one launch (one block per (sample, channel block); c / groups in
 * {1, 2, 4, 8}; pool 1 or 2): statistics from the conv's stat_partials [n][tiles][c8*8][2], written to stats_ng2 for the
 * backward pass, and a = act(GN(y)) [+ AvgPool2d(pool)]. */
int mc_gn_act_fwd_small(const void* y, const float* stat_partials, int32_t tiles, int32_t n, int32_t c, int32_t h, int32_t w,
                        int32_t groups, float eps, const float* gamma, const float* beta, int32_t act, int32_t pool,
                        int32_t dtype, float* stats_ng2, void* a, void* pooled, void* stream);
/* Backward of act(GN(y)) given the gradient sources of a.  Phase 1 reduces
 * (sum dz, sum dz*yhat) per (n,c) into partials [n][blocks][c8*8][2]; phase 2 (finalize)
 * turns them into per-(n,g) means and accumulates dgamma/dbeta (in sample order: deterministic); phase 3 writes dy. */
int32_t mc_gn_bwd_blocks(int32_t h, int32_t w);
int mc_gn_act_bwd_reduce(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                         const float* stats_ng2, const float* gamma, const float* beta, int32_t post,
                         int32_t act, int32_t dtype, const mc_grad_src* g0, const mc_grad_src* g1,
                         float* partials, void* stream);
int mc_gn_act_bwd_finalize(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups,
                           int32_t hw, const float* gamma, float* m12_ng2, float* dgamma, float* dbeta,
                           void* stream);
/* The same for partial tables with many slots per sample (the input-gradient epilogue's): one block per (group, sample);
 * writes m12 [n][groups][2] and the per-(sample, channel) sums chan_sums [n][c8*8][2]; dgamma / dbeta follow from
 * mc_gn_param_grads_batched (samples in order: deterministic).  Channels per group: 1, 2, 4 or 8. */
int mc_gn_act_bwd_finalize_n(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                             const float* gamma, float* m12_ng2, float* chan_sums, void* stream);
/* The two finalize forms, writing in addition the table mc_conv2d_wgrad_dz reads: dz_coef [n][c8*8][4] = (cA, cB, cC, mean)
 * per (sample, channel) from coef (the layer's (scale, shift, mean, rstd) table) and the m12 just computed; rows of padded
 * channels are not written (allocate the table zeroed).  m12_ng2 is required. */
int mc_gn_act_bwd_finalize_dz(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                              const float* gamma, float* m12_ng2, float* dgamma, float* dbeta, const float* coef,
                              float* dz_coef, void* stream);
int mc_gn_act_bwd_finalize_n_dz(const float* partials, int32_t n, int32_t blocks, int32_t c, int32_t groups, int32_t hw,
                                const float* gamma, float* m12_ng2, float* chan_sums, const float* coef, float* dz_coef,
                                void* stream);
int mc_gn_act_bwd_apply(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                        const float* stats_ng2, const float* m12_ng2, const float* gamma,
                        const float* beta, int32_t post, int32_t act, int32_t dtype,
                        const mc_grad_src* g0, const mc_grad_src* g1, void* dy, void* stream);
/* Small layers: the three phases in one launch (one block per (sample, channel block); needs c / groups in {1, 2, 4, 8}).
 * Writes dy and the per-(sample, channel) sums chan_sums [n][ceil(c/8)*8][2] = (sum dz, sum dz * yhat); dgamma / dbeta are
 * accumulated from those tables, samples in order, by mc_gn_param_grads_batched (one launch for many layers: per-layer
 * tables are plain host arrays of length `jobs`). */
int mc_gn_act_bwd_small(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats_ng2,
                        const float* gamma, const float* beta, int32_t act, int32_t dtype, const mc_grad_src* g0,
                        const mc_grad_src* g1, void* dy, float* chan_sums, void* stream);
int mc_gn_param_grads_batched(const float* const* chan_sums, const int32_t* n, const int32_t* c, float* const* dgamma,
                              float* const* dbeta, int32_t jobs, void* stream);
/* ---- Dropout after the activation (nn.Dropout at the end of a FluidLayer, :753, :798) -------
 * a_drop = a * m * s, element-wise.  An element is kept (m = 1) with probability keep16 / 65536, keep16 =
 * clamp(round((1 - p) * 65536), 1, 65535), s = f32(65536 / keep16): the rate is quantised to 2^-16.  The mask is a pure
 * function of (seed, step, layer, logical element) -- Philox4x32-10 with key (seed_lo, seed_hi) and counter (v_lo, v_hi,
 * layer, step), v = ((n * c8 + cb) * h + y) * w + x the 64-bit index of the CB8 vector; channel j of the vector takes the
 * 16-bit field (out[j >> 1] >> 16 (j & 1)) & 0xffff and is kept iff field < keep16 -- so it does not depend on dtype, kernel
 * or launch shape, and the backward pass regenerates it instead of reading a stored mask.
 * state: device uint32[4] = (seed_lo, seed_hi, step, 0), read by the kernels when they run (a replayed HIP graph sees the
 * current step); mc_dropout_advance adds 1 to state[2] with a one-thread kernel on `stream`. */
typedef struct {
  const uint32_t* state;
  uint32_t layer;
  uint32_t keep16;
} mc_dropout;
int mc_dropout_advance(uint32_t* state, void* stream);
/* The existing entry points with dropout: forward multiplies the f32 activation by m * s before the store rounding, backward
 * multiplies the f32 sum of the gradient sources by m * s before act'.  Lanes past c stay zero.  pool must be 1
 * (MC_EUNSUPPORTED otherwise: a dropout layer is never pooled in its own launch); drop == NULL or keep16 outside
 * [1, 65535] is MC_EINVAL.  The backward forms take every gradient-source kind (the trunk's first layer of NewFluidNet sums
 * a conv's and a pooling level's gradients). */
int mc_gn_act_fwd_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                       const float* stats_ng2, const float* gamma, const float* beta, int32_t post,
                       int32_t act, int32_t pool, int32_t dtype, void* a, void* pooled, const mc_dropout* drop, void* stream);
int mc_gn_act_fwd_small_drop(const void* y, const float* stat_partials, int32_t tiles, int32_t n, int32_t c, int32_t h, int32_t w,
                             int32_t groups, float eps, const float* gamma, const float* beta, int32_t act, int32_t pool,
                             int32_t dtype, float* stats_ng2, void* a, void* pooled, const mc_dropout* drop, void* stream);
int mc_gn_act_bwd_reduce_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                              const float* stats_ng2, const float* gamma, const float* beta, int32_t post,
                              int32_t act, int32_t dtype, const mc_grad_src* g0, const mc_grad_src* g1,
                              float* partials, const mc_dropout* drop, void* stream);
int mc_gn_act_bwd_apply_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                             const float* stats_ng2, const float* m12_ng2, const float* gamma,
                             const float* beta, int32_t post, int32_t act, int32_t dtype,
                             const mc_grad_src* g0, const mc_grad_src* g1, void* dy, const mc_dropout* drop, void* stream);
int mc_gn_act_bwd_small_drop(const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups, const float* stats_ng2,
                             const float* gamma, const float* beta, int32_t act, int32_t dtype, const mc_grad_src* g0,
                             const mc_grad_src* g1, void* dy, float* chan_sums, const mc_dropout* drop, void* stream);
/* Host twins of the generator the kernels inline (no device needed): Philox4x32-10 itself, and the keep flags (0 / 1) of the
 * 8 channels of the vectors first_vec .. first_vec + n_vec - 1 into out[n_vec * 8]. */
void mc_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
int mc_dropout_mask_host(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t layer, uint64_t first_vec, uint64_t n_vec,
                         uint32_t keep16, uint8_t* out);
/* Phase 3 for a tensor whose dz = dA * act'(z) was already written by mc_conv2d_fused's epilogue (+ mc_fold_padded_dz):
 * dy = scale * dz - rstd (m1 + yhat m2)  (coef = the layer's table, m12 from mc_gn_act_bwd_finalize); with coef == NULL
 * (activation-only layer) dy = dz.  dz is read through a gradient source (MC_GSRC_PADFOLD or MC_GSRC_PLAIN). */
int mc_gn_bwd_apply_dz(const mc_grad_src* dz, const void* y, int32_t n, int32_t c, int32_t h, int32_t w, int32_t groups,
                       const float* coef, const float* m12_ng2, int32_t dtype, void* dy, void* stream);
/* ---- torch.cat of up to 12 operands along channels (NewFluidNet.forward, pytorch_networks_convae.py:1327-1332; the Unet's
 * skip concats): out [n][ceil(sum C / 8)][h][w][8], operand k at channels [sum_{j<k} C_j, + C_k).  Any channel counts; when
 * every operand but the last is a multiple of 8 the launch is a copy of whole blocks.  The lanes past the last channel are
 * written as zeros when some operand is not a multiple of 8 (when all are aligned they are copied from the last operand). */
int mc_concat_cb8(const void* const* srcs, const int32_t* src_c, int32_t n_src, int32_t n, int32_t h, int32_t w,
                  int32_t dtype, void* out, void* stream);
/* Gradient of one concat operand that does not fill whole blocks of the concatenated tensor: out (plain CB8 [n][ceil(c/8)]
 * [h][w][8], lanes past c zero) = channels [c_off, c_off + c) of the gradient of the c_total-channel concatenated tensor, read
 * through g (MC_GSRC_PLAIN or MC_GSRC_PADFOLD, a whole tensor: c8_total == 0, hs x ws == h x w).  dtype: the gradient type. */
int mc_cat_grad_gather(const mc_grad_src* g, int32_t c_total, int32_t c_off, int32_t c, int32_t n, int32_t h, int32_t w,
                       int32_t dtype, void* out, void* stream);
/* out (plain CB8 [n][c/8][h][w][8]) = g0 + g1: materialises the gradient of a tensor with two consumers
 * (the pooled feature maps of NewFluidNet feed a conv AND the next pooling level). */
int mc_gsrc_sum(const mc_grad_src* g0, const mc_grad_src* g1, int32_t n, int32_t c, int32_t h, int32_t w,
                int32_t dtype, void* out, void* stream);

/* Rectangle copy between CB8 tensors of the same channel count: dst[n][cb][dy+r][dx+c] (=|+=) src[n][cb][sy+r][sx+c] for
 * r < rh, c < rw; src == NULL writes zeros.  Used to cut the border strips of BoundaryLearnedConvolution2D out of its input
 * and to frame its output (pytorch_networks_convae.py:1022-1065). */
int mc_rect_copy(const void* src, int32_t hs, int32_t ws, int32_t sy, int32_t sx, void* dst, int32_t hd, int32_t wd,
                 int32_t dy, int32_t dx, int32_t rh, int32_t rw, int32_t n, int32_t c, int32_t accumulate, int32_t dtype,
                 void* stream);

/* ---- learned padding: the FRAME of BoundaryLearnedConvolution2D (pytorch_networks_convae.py:1022-1065) --------------
 * The layer is nine bias-free valid convolutions: the main bank on the whole input and eight border banks on the strips of
 * width pad = k + 1 + (bc - 1) (k = 5) or k + (bc - 1) (k = 3), framed around the main result, plus one shared bias.  With
 * f = pad - k + 1, mh = h - k + 1, mw = w - k + 1 the output is (mh + 2 fy) x (mw + 2 fx); the frame is every output pixel
 * outside the mh x mw interior at (fy, fx).  The main bank runs on mc_conv2d / mc_conv2d_wgrad; the entry points below
 * compute the frame of all eight border banks in ONE launch per direction, reading x / dy in place.
 *   row class:    oy < fy: "bottom", window origin iy0 = h - pad_y + oy (the strip cut from the LAST input rows lands in the
 *                 FIRST output rows, :1057-1060);  oy >= fy + mh: "top", iy0 = oy - (fy + mh);  else middle, iy0 = oy - fy
 *   column class: ox < fx: "left", ix0 = ox;  ox >= fx + mw: "right", ix0 = w - pad_x + (ox - fx - mw);  else ix0 = ox - fx
 * Bank arrays (w_unique, dw_unique) hold the eight border banks in the order
 *   bottom_left, bottom, bottom_right, left, right, top_left, top, top_right
 * each in the reference's layout [U][c_in][k][k] f32 (U = c_out - sym_h / 2 unique filters).
 * dtype as everywhere: MC_MIX16 reads x / writes y as f16 and moves dy / dx as bf16. */
typedef struct {
  int32_t n;
  int32_t h, w;        /* INPUT spatial size */
  int32_t c_in, c_out; /* any counts; tail channels of a CB8 block are read as zero and stored as zero */
  int32_t k;           /* 3 or 5 */
  int32_t bc_x, bc_y;  /* >= 1: widen the strips by bc - 1 (the output grows) */
  int32_t dtype;       /* MC_F32 | MC_BF16 | MC_MIX16 */
  int32_t sym_h;       /* number of x-mirrored filters of every bank (even), 0 = plain Conv2d */
} mc_learned_desc;

/* Host-side check (needs no device): MC_OK, MC_EINVAL (NULL / non-positive sizes) or MC_EUNSUPPORTED for k not in {3, 5},
 * h < pad_y, w < pad_x, h < k, w < k, an odd sym_h or an unknown dtype.  Every entry point below runs it first, so an input
 * that is too small for the strips is refused before any launch. */
int32_t mc_learned_validate(const mc_learned_desc* d);
/* Bytes of the packed banks of all eight border banks (dgrad = 0: forward, 1: input gradient) and of the filter-gradient
 * workspace; 0 for a descriptor mc_learned_validate refuses. */
size_t mc_learned_bank_bytes(const mc_learned_desc* d, int32_t dgrad);
size_t mc_learned_wgrad_workspace_bytes(const mc_learned_desc* d);
/* Pack the border banks of n layers in batched launches: w_unique[8 * i + b] is bank b of layer i; fwd_banks[i] and
 * dgrad_banks[i] (the array or an entry may be NULL: no input gradient) receive mc_learned_bank_bytes each. */
int mc_learned_pack_banks_batched(const mc_learned_desc* descs, const float* const* w_unique, void* const* fwd_banks,
                                  void* const* dgrad_banks, int32_t n, void* stream);
/* y[frame] = bias + W_bank * x.  x: CB8 [n][c_in8][h][w]; y: CB8 [n][c_out8][ho][wo].  Elements of y outside the frame are
 * not written. */
int mc_learned_frame_fwd(const mc_learned_desc* d, const void* x, const void* fwd_bank, const float* bias, void* y,
                         void* stream);
/* dx += the eight border banks' input gradients (dx already holds the main bank's).  A gather over the input pixels of
 * the border bands (rows < pad_y or >= h - pad_y, columns < pad_x or >= w - pad_x): each pixel is owned by one thread that
 * sums every bank's contribution, so the result does not depend on block order; pixels outside the bands are not written. */
int mc_learned_frame_dgrad(const mc_learned_desc* d, const void* dy, const void* dgrad_bank, void* dx, void* stream);
/* dw_unique[b] += filter gradient of border bank b (mirrored filters folded back), dbias += the sum of dy over the frame.
 * Two launches: per-slice partial slabs into `workspace`, then a reduce in fixed order (bit-reproducible). */
int mc_learned_frame_wgrad(const mc_learned_desc* d, const void* x, const void* dy, void* workspace,
                           float* const* dw_unique, float* dbias, void* stream);

/* ---- resampling (nn.AvgPool2d, nn.Upsample(mode='bicubic'); Unet :2002,2009,2014; ConvAE :1051,1079) */
int mc_avgpool_fwd(const void* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t f, int32_t dtype,
                   void* out, void* stream);
/* taps: idx [out][4] int32 (clamped), wgt [out][4] f32, per axis (host-built in f64, A = -0.75). */
int mc_bicubic_fwd(const void* x, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                   const int32_t* idx_y, const float* wgt_y, const int32_t* idx_x, const float* wgt_x,
                   int32_t dtype, void* out, void* stream);
/* mc_bicubic_fwd of act(scale * x + shift): x is a raw conv output, activated while the input window is staged
 * (coef nullable = activation only). */
int mc_bicubic_fwd_act(const void* x, const float* coef, int32_t act, int32_t n, int32_t c, int32_t hi, int32_t wi,
                       int32_t ho, int32_t wo, const int32_t* idx_y, const float* wgt_y, const int32_t* idx_x,
                       const float* wgt_x, int32_t dtype, void* out, void* stream);
/* adjoint: transposed tap tables in CSR form per axis (start [in+1], j [], w []). */
int mc_bicubic_bwd(const mc_grad_src* g, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                   const int32_t* ty_start, const int32_t* ty_j, const float* ty_w,
                   const int32_t* tx_start, const int32_t* tx_j, const float* tx_w,
                   int32_t dtype, void* dx, void* stream);
/* The same with the longest tap list of each table given (host knowledge of the tables; 0 = unknown): lists of <= 8 entries
 * (every even x2 upsample) run a kernel instantiation that holds 8 instead of 12 taps per pixel on chip. */
int mc_bicubic_bwd_taps(const mc_grad_src* gs, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                        const int32_t* tys, const int32_t* tyj, const float* tyw, const int32_t* txs, const int32_t* txj,
                        const float* txw, int32_t max_taps_y, int32_t max_taps_x, int32_t dtype, void* dx, void* stream);
/* The same adjoint as a walk down the output rows (each read once into registers; a sliding register window of the four
 * open input rows; one LDS crossing per finished row for the x taps): takes the FORWARD y tables (idx_y, wgt_y: [ho][4], as
 * mc_bicubic_fwd) plus the transposed lists (ty_start / ty_j for the chunk extents, the x lists for the gather).  Any ratio
 * ho / hi >= 1; x tap lists of <= 12 entries (max_taps_x: the longest, host knowledge of the table), else MC_EUNSUPPORTED. */
int mc_bicubic_bwd_walk(const mc_grad_src* gs, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                        const int32_t* idx_y, const float* wgt_y, const int32_t* tys, const int32_t* tyj, const int32_t* txs,
                        const int32_t* txj, const float* txw, int32_t max_taps_x, int32_t dtype, void* dx, void* stream);
/* The same adjoint as two 1-D passes through an f32 workspace [n][ceil(c/8)][hi][wo][8]: for large scale factors
 * (NewFluidNet upsamples x4 ... x16 to the full grid, pytorch_networks_convae.py:1239-1244), where a pixel's tap lists
 * are too long for the tiled kernel. */
int mc_bicubic_bwd_separable(const mc_grad_src* g, int32_t n, int32_t c, int32_t hi, int32_t wi, int32_t ho, int32_t wo,
                             const int32_t* ty_start, const int32_t* ty_j, const float* ty_w,
                             const int32_t* tx_start, const int32_t* tx_j, const float* tx_w,
                             int32_t dtype, float* ws, void* dx, void* stream);

/* ---- curl head (Unet :2038-2070): a*a_bound -> u = da/dy, v = -da/dx, antisymmetric walls;
 *      optional T = clip(t_in, t_lo, t_hi) (:2040).  Planes are [h][w] f32 with a batch stride. --- */
int mc_curl_head_fwd(const float* a, const float* t_in, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride,
                     float a_bound, float t_lo, float t_hi, float* u, float* v, float* t_out, void* stream);
/* ws: workspace of 2*n*(h-2)*(w-2) floats.  ga / gt_in: gradients w.r.t. a / t_in (same batch stride). */
int mc_curl_head_bwd(const float* gu, const float* gv, const float* gt_out, const float* t_in, int32_t n, int32_t h,
                     int32_t w, float a_bound, float t_lo, float t_hi, float* ga, float* gt_in,
                     int64_t g_batch_stride, int64_t in_batch_stride, float* ws, void* stream);

/* ---- curl head of FluidNet (pytorch_networks_convae.py:1681-1697): a = a_bound * y[:, 0] on an (h+2) x (w+2) field,
 *      u[i][j] = 0.5 (a[i+2][j+1] - a[i][j+1]), v[i][j] = -0.5 (a[i+1][j+2] - a[i+1][j]) on h x w, no wall fix-up.
 *      a / ga: (h+2) x (w+2) f32 planes with a batch stride; u, v, gu, gv: [n][h][w].  The backward writes every pixel of
 *      ga's planes (no memset needed) without atomics or workspace. --- */
int mc_curl_valid_fwd(const float* a, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride, float a_bound, float* u,
                      float* v, void* stream);
int mc_curl_valid_bwd(const float* gu, const float* gv, int32_t n, int32_t h, int32_t w, float a_bound, float* ga,
                      int64_t g_batch_stride, void* stream);

/* ---- blurred streamfunction (`-blurr 1`; NewFluidNet :1357-1361, FluidNet :1682-1686): the four heads above with
 *      A = a_bound * a replaced by its 3 x 3 box mean over the replicate-padded plane the head reads (hp x wp = h x w for the
 *      wall form, (h+2) x (w+2) for the valid form):
 *        B[i][j] = wb * sum_{di, dj in {-1,0,1}} A[clamp(i+di, 0, hp-1)][clamp(j+dj, 0, wp-1)],  wb = 1.0f / 9.0f (the f32 value);
 *      u, v are what the unblurred twin makes of B (wall form: corners exactly 0; t_out = clip(t_in) as before, T is not
 *      blurred).  The adjoints are the transposes: the clamped mean is symmetric, so ga is the same clamped 3 x 3 sum of the
 *      twin's stencil adjoint.  The mean is fused: forward is one launch (plus the clip when t_in is given), backward the
 *      twin's launches (fold + gather / one gather), B and its gradient never reach memory, every output pixel is written
 *      once, no atomics (bit-reproducible).  Arguments, batch strides, workspace size and MC_EINVAL cases are the twins';
 *      all four also return MC_EINVAL for n > 65535 (the batch is a grid dimension). --- */
int mc_curl_blur_head_fwd(const float* a, const float* t_in, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride,
                          float a_bound, float t_lo, float t_hi, float* u, float* v, float* t_out, void* stream);
int mc_curl_blur_head_bwd(const float* gu, const float* gv, const float* gt_out, const float* t_in, int32_t n, int32_t h,
                          int32_t w, float a_bound, float t_lo, float t_hi, float* ga, float* gt_in,
                          int64_t g_batch_stride, int64_t in_batch_stride, float* ws, void* stream);
int mc_curl_blur_valid_fwd(const float* a, int32_t n, int32_t h, int32_t w, int64_t in_batch_stride, float a_bound, float* u,
                           float* v, void* stream);
int mc_curl_blur_valid_bwd(const float* gu, const float* gv, int32_t n, int32_t h, int32_t w, float a_bound, float* ga,
                           int64_t g_batch_stride, void* stream);

/* ---- loss (Trainer.loss_fn multigpu.py:122-134; get_loss :250-305) + build-defined momentum -- */
#define MC_LOSS_SLOTS 16
enum { MC_S_U_SCALED = 0, MC_S_U_PLAIN, MC_S_V_SCALED, MC_S_V_PLAIN, MC_S_P_PLAIN, MC_S_T_PLAIN,
       MC_S_DU, MC_S_DV, MC_S_MASS, MC_S_MASS_X0, MC_S_MASS_X1, MC_S_MASS_Y0, MC_S_MASS_Y1,
       MC_S_MOMX, MC_S_MOMY, MC_S_SPARE };
typedef struct {
  int32_t n, h, w;
  int32_t p_pred;          /* uvp = (u,v,p,T) if p_pred else (u,v,T)                      */
  int32_t loss_type;       /* 0 mae, 1 mass, 2 curl                                        */
  int32_t loss_scale;      /* Trainer.loss_scale                                           */
  int32_t loss_derivative; /* Trainer.loss_derivative                                      */
  int32_t l2;              /* 0: L1 (reference); 1: squared error for the data terms       */
  float lambda_mom;        /* weight of the momentum residual term (0 = off)               */
  float inv_h;             /* 1/h of the momentum residual (126).  NOT used by the derivative */
                           /* terms: their x126 is the reference's literal (multigpu.py:163-166) */
  float ra;                /* Rayleigh number in the buoyancy term (1)                     */
  int32_t t_grad;          /* 1: T is a network output (gets a gradient); 0: T is given;   */
                           /* -1: the network has no temperature output (FluidNet family,  */
                           /* multigpu.py:138-195): T / gT may be NULL, uvp is (u, v[, p]) */
                           /* -2: as -1, with the temperature term of the advection step   */
                           /* (mc_advect_loss) as one more term of the average             */
} mc_loss_desc;
/* per-sample (min, max) over (H,W) of the truth channels u, v and (when ct >= 3) channel 2: mm [n][3][2] */
int mc_loss_minmax(const float* uvp, int32_t n, int32_t ct, int32_t h, int32_t w, float* mm, void* stream);
/* Fused forward + backward of the data / derivative / divergence terms.  u,v,p,T: predictions
 * [n][h][w] f32 with the given batch strides (p may be NULL); sums: MC_LOSS_SLOTS doubles
 * (zeroed by the caller); gu..gT: d(loss)/d(pred), same strides as the predictions (p and gp
 * use p_batch_stride: in curl mode p is a channel of the network output while u, v, T come
 * from the curl head) (overwritten).  The momentum term is added by mc_momentum_* below. */
int mc_loss_fwd_bwd(const mc_loss_desc* d, const float* u, const float* v, const float* p, const float* T,
                    int64_t pred_batch_stride, int64_t p_batch_stride, const float* uvp, const float* mm,
                    double* sums, float* gu, float* gv, float* gp, float* gT, void* stream);
/* mc_loss_fwd_bwd + mc_momentum_residual + mc_momentum_adjoint in ONE launch (the residual signs and the viscosity stay in
 * LDS), for the Unet branch without the curl head (loss_type 0 / 1, t_grad >= 0; else MC_EUNSUPPORTED).  The predictions come
 * either as planes (u, v, p, T with batch strides, as mc_loss_fwd_bwd; y_cb8 NULL) or straight from the last convolution's
 * f32 output y_cb8 [n][ceil(cb8_c / 8)][h][cb8_w][8]: columns cb8_crop .. cb8_crop + w, minus cb8_mean [n][cb8_c] (nullable),
 * channels u, v, T, p = 0, 1, 2, 3 (Unet.forward :2026-2036) -- which saves the NCHW copy of the network output.  yc [h][w],
 * paras [n][3], scaler [n] are read when lambda_mom != 0.  Gradients: planes with batch strides g_pbs / g_ppbs
 * (overwritten). */
int mc_loss_fused(const mc_loss_desc* d, const float* u, const float* v, const float* p, const float* T, int64_t pbs, int64_t ppbs,
                  const float* y_cb8, int32_t cb8_w, int32_t cb8_crop, const float* cb8_mean, int32_t cb8_c, const float* uvp,
                  const float* mm, const float* yc, const float* paras, const float* scaler, double* sums, float* gu, float* gv,
                  float* gp, float* gT, int64_t g_pbs, int64_t g_ppbs, float* gsum_part, void* stream);
/* gsum_part (nullable): [n][mc_loss_fused_blocks(n, h, w)][4] per-block sums of the gradient planes (u, v, T, p; deterministic
 * order); mc_partial_sums_finalize turns them into out[n * c + j] = scale * (sum over the blocks), j < c <= 4 -- the spatial
 * means the adjoint of the network's mean subtraction needs (mc_pack_grad_nchw), without a pass over the gradient tensor. */
int32_t mc_loss_fused_blocks(int32_t n, int32_t h, int32_t w);
int mc_partial_sums_finalize(const float* part, int32_t n, int32_t blocks, int32_t c, float scale, float* out, void* stream);
/* Stokes momentum residual (build-defined).  yc [h][w], paras [n][3] =
 * (RaQ, FKT, FKP), scaler [n].  sx, sy, eta_ws: workspaces [n][h][w] f32 (eta_ws receives the viscosity
 * field computed by mc_momentum_residual and is read again by mc_momentum_adjoint). */
int mc_momentum_residual(const mc_loss_desc* d, const float* u, const float* v, const float* p,
                         const float* T, int64_t pred_batch_stride, int64_t p_batch_stride, const float* yc, const float* paras,
                         const float* scaler, double* sums, float* sx, float* sy, float* eta_ws, void* stream);
int mc_momentum_adjoint(const mc_loss_desc* d, const float* T, int64_t pred_batch_stride, int64_t p_batch_stride, const float* eta_ws,
                        const float* paras, const float* scaler, const float* sx, const float* sy,
                        float* gu, float* gv, float* gp, float* gT, void* stream);
/* loss6 (+momentum) from the sums, exactly as get_loss combines them: out[8] f32 =
 * (loss, loss_true_u, loss_true_v, loss_p, loss_T, mean mass, mom, 0). */
int mc_loss_finalize(const mc_loss_desc* d, const double* sums, float* out8, void* stream);
/* Advection loss (build-defined, the reference's `-ad 1`; DESIGN.md 9 "Advection loss"): the temperature term of the FluidNet
 * family.  Item b of x [n][x_channels >= 7][h][w] = (xc/4, yc/4, log10 eta/8, nd0, nd1, nd2, T) carries its own grid
 * X = 4 x[0], Y = 4 x[1] (wall coordinates 0 / 4 and 0 / 1 substituted as mc_adnet_step does) and temperature T = x[6];
 * uvp [n][uvp_channels][h][w] = truth (u, v[, p]), scaler [n] = s.
 * mc_advect_loss_dt: dt[b] = fminf(0.5f cn_max dx_min_b / uv_b, 0.5f dx2 dx2 / (dx2 + dx2)), dx2 = dx_min_b^2, with dx_min_b
 * the smallest interior X[i][j] - X[i][j-1] and uv_b = max(|s u_t|, |s v_t|) over the interior of item b -- mc_adnet_step's
 * f32 expression, bit-identical to mc_rollout_dx_min + mc_rollout_dt on a shared grid; an item at rest gets the diffusive
 * limit.  ws: MC_ADVECT_WS_PER_ITEM n uint32 scratch (per-workgroup partial maxima and minima; nothing to reset).
 * mc_advect_loss (d->t_grad == -2; after mc_loss_fwd_bwd, before mc_loss_finalize): with A(u, v) = -u Dx(u) - v Dy(v), the
 * upwind differences of T of ADNet.forward, e = dt[b] (A(s u_p, s v_p) - A(s u_t, s v_t)) on the interior;
 * sums[MC_S_T_PLAIN] += sum |e| (1 + [j == 1] + [j == w-2])  (e^2 with d->l2) -- l1(ADNet(pred), ADNet(true)) at the given dt
 * once mc_loss_finalize divides by n h w -- and d(loss)/d(u_p, v_p) is ADDED to the interior of gu, gv (batch stride
 * pred_batch_stride, as u, v); their boundary rows and columns are not touched.  u_p == 0 contributes exactly 0.
 * Both return MC_EINVAL, launching nothing, for a null pointer, n <= 0 or n > 65535, h < 5, w < 5 or x_channels < 7. */
#define MC_ADVECT_WS_PER_ITEM 64
int mc_advect_loss_dt(const float* uvp, int32_t uvp_channels, const float* x, int32_t x_channels, const float* scaler,
                      int32_t n, int32_t h, int32_t w, float cn_max, uint32_t* ws, float* dt, void* stream);
int mc_advect_loss(const mc_loss_desc* d, const float* u, const float* v, int64_t pred_batch_stride, const float* uvp,
                   const float* x, int32_t x_channels, const float* scaler, const float* dt, double* sums, float* gu, float* gv,
                   void* stream);

/* ---- on-device batch assembly (ADTimeDataset.__getitem__, datasetio.py:229-280) -----------------
 * The whole dataset stays resident in HBM: T [m][h][w], uv [m][cy][h][w] (cy >= 2: u, v[, p]), t [m], paras [m][3] =
 * (RaQ, FKT, FKP), paras_nd [m][3], xc / yc [h][w], all f32.  For every (i0, i1) of pairs [b][2] writes
 *   x [b][10][h][w] = (xc, yc, t[i1]-t[i0], paras_nd[i0] x3, log10(clip(eta,1e-8,1))/8, T[i0], u[i0]/s, v[i0]/s)
 *   y [b][3][h][w]  = (u[i1]/s, v[i1]/s, T[i1]),  scaler [b] = s,  paras_out [b][3] = paras[i0]
 * with s = 5 exp(1.80167667 RaQ/10 + 0.4330392 ln FKT - 0.46052953 ln FKP) (scaler.py:6-13) and
 * eta = exp(-ln(FKT) T + ln(FKP) (1 - yc)) (pytorch_networks_convae.py:86-102). */
int mc_assemble_adtime_batch(const float* T, const float* uv, const float* t, const float* paras, const float* paras_nd,
                             const float* xc, const float* yc, const int32_t* pairs, int32_t b, int32_t m, int32_t cy,
                             int32_t h, int32_t w, float* x, float* y, float* scaler, float* paras_out, void* stream);

/* The FluidNet family's dataset (NewADDataset.__getitem__, datasetio.py:595-654), same residency: T [m][h][w], uvp
 * [m][cy][h][w] (cy = 2 or 3: u, v[, p]), t [m] (the item's time weight).  For every item idx[b] writes
 *   x [b][7][h][w] = (xc/4, yc/4, log10(clip(eta,1e-8,1))/8, paras_nd x3, T),  y [b][cy][h][w] = (u/s, v/s[, p]),
 *   t_weight [b] = t[idx], scaler [b] = s.  (No input noise here: mc_assemble_newad_step applies the reference's.) */
int mc_assemble_newad_batch(const float* T, const float* uvp, const float* t, const float* paras, const float* paras_nd,
                            const float* xc, const float* yc, const int32_t* idx, int32_t b, int32_t m, int32_t cy,
                            int32_t h, int32_t w, float* x, float* y, float* t_weight, float* scaler, void* stream);

/* ---- resident epoch loop: the batch is assembled inside the (captured) step ------------------------------------
 * One item store = the resident arrays of one dataset, as the batch entry points above take them (uv [m][cy][h][w]). */
typedef struct {
  const float *T, *uv, *t, *paras, *paras_nd, *xc, *yc;
  int32_t m;
} mc_item_store;
/* The item arithmetic of mc_assemble_*_batch (the same device functions: equal bits for equal items) with the indices read on
 * the device: table int32 [rows][b] (ADTime: [rows][b][2]) is one epoch's batches, cursor uint32[4] = (step, steps, draw, 0)
 * chooses row `step`; both pointers and the outputs are fixed, so one captured launch serves every replay.  An entry e >= 0
 * is item e of main_store, e < 0 item -e - 1 of init_store (ADTime: the sign of a pair's first entry decides for both);
 * init_store may be NULL when the table has no negative entry.  A cursor outside the table or an entry outside its store
 * writes nothing for that row / batch slot (the host validates tables before upload).
 * noise != 0 (NewAD; reference datasetio.py:604-613, which draws U(-1e-5, 1e-5) whatever the value): on the interior
 * [2:h-2, 2:w-2]  T <- clip(T + n, 0, 1.35), the two-pixel frame keeps T, the viscosity channel follows the noisy T, the
 * targets are unchanged.  n = (2u - 1) 1e-5, u = ((bits >> 8) + 0.5) 2^-24, bits = word 0 of Philox4x32-10 with key (seed_lo,
 * seed_hi) and counter (pixel y * w + x, item | 0x80000000 for the init store, cursor draw, 0x6e6f6973): a pure function of
 * (seed, draw, item, pixel), independent of launch shape and batch position. */
int mc_assemble_adtime_step(const mc_item_store* main_store, const mc_item_store* init_store, const int32_t* table,
                            const uint32_t* cursor, int32_t rows, int32_t b, int32_t cy, int32_t h, int32_t w, float* x, float* y,
                            float* scaler, float* paras_out, void* stream);
int mc_assemble_newad_step(const mc_item_store* main_store, const mc_item_store* init_store, const int32_t* table,
                           const uint32_t* cursor, int32_t rows, int32_t b, int32_t cy, int32_t h, int32_t w, int32_t noise,
                           uint32_t seed_lo, uint32_t seed_hi, float* x, float* y, float* t_weight, float* scaler, void* stream);
/* One-thread kernel on `stream`: step = (step + 1) % steps, draw += 1.  Launched after the assembly, so every replay of a
 * captured step consumes one table row and one noise draw. */
int mc_loader_advance(uint32_t* cursor, void* stream);
/* Host twin of the noise the kernel inlines (no device needed); item carries the store bit. */
float mc_newad_noise_host(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t item, uint32_t pixel);

/* ---- Trainer.get_loss with roll_forward = R > 1 (multigpu.py:207-248): the network is applied R * R times in a chain, each
 * input rebuilt from channels 0..5 of the batch and the previous evaluation's T, u, v.  x [n][c][h][w] f32 (c >= 10) holds the
 * batch's RAW channels (the input-pack kernel applies xc / 4, yc / 4, dt / R); this call overwrites channels 7, 8, 9 with t, u,
 * v ([h][w] planes with a batch stride: the curl head's outputs or channels of the network output) and, when update_v != 0
 * (after a pre-step; the reference leaves V alone after a round's last step, :246-247), channel 6 with
 * log10(clip(exp(-ln(FKT) t + ln(FKP) (1 - yc)), 1e-8, 1)) / 8, yc = channel 1 of x; paras [n][3] = (RaQ, FKT, FKP). */
int mc_roll_forward_update(float* x, int32_t c, const float* u, const float* v, const float* t, int64_t uvt_batch_stride,
                           const float* paras, int32_t update_v, int32_t n, int32_t h, int32_t w, void* stream);

/* ---- inference rollout (TS.forward / ADNet.forward, pytorch_networks_convae.py:266-568) ----------
 * Input builder of the 'newfluidnet' branch (:372-395): out [n][7][h][w] = (xc/4, yc/4, log10(clip(eta,1e-8,1))/8, nd0, nd1,
 * nd2, T) with eta = exp(-ln(FKT) T + ln(FKP) (1 - ycc)); T [n][h][w], xc/yc/ycc [h][w], paras [n][3] = (RaQ, FKT, FKP),
 * paras_nd [n][3]. */
int mc_ts_build_input(const float* T, const float* xc, const float* yc, const float* ycc, const float* paras,
                      const float* paras_nd, int32_t n, int32_t h, int32_t w, float* out, void* stream);
/* Input builder of the 'unet' branch (:411-436): out [n][10][h][w] = (xc/4, yc/4, dt, nd0, nd1, nd2,
 * log10(clip(eta,1e-8,1))/8, T, u_prev, v_prev); dt, u_prev, v_prev [n][h][w].  The network predicts the next T itself;
 * mc_ts_wall_bc applies the wall rows (bottom 1, top 0) and copies the side columns from their inner neighbours
 * (:441-444) out of place. */
int mc_ts_build_input_unet(const float* T, const float* xc, const float* yc, const float* ycc, const float* paras,
                           const float* paras_nd, const float* dt, const float* u_prev, const float* v_prev, int32_t n,
                           int32_t h, int32_t w, float* out, void* stream);
int mc_ts_wall_bc(const float* t_in, int32_t n, int32_t h, int32_t w, float* t_out, void* stream);
/* One explicit upwind advection-diffusion step (ADNet.forward :522-568) on the non-uniform grid xc / yc [h][w] (wall
 * coordinates 0 / 4 and 0 / 1 are substituted on the fly, as the reference writes them into its inputs): u, v [n][h][w]
 * with batch stride uv_stride, multiplied by vel_scale[n] (NULL = 1: TS un-scales the network's velocities, :397-398);
 * raq_field [n][h][w] or NULL with raq_scalar[n]; dt_io: device scalar; compute_dt != 0 -> the CFL step
 * min(0.5 CN_max dx_min / max|u,v|, dx_min^2 / 4) is computed into it first (ws: 2 x uint32 scratch), else it is read.
 * T_next [n][h][w]: interior updated, replicate-padded, first row 1, last row 0 (side columns = their neighbours, which
 * is also TS's side condition :466-469). */
int mc_adnet_step(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* T_prev,
                  const float* raq_field, const float* raq_scalar, const float* xc, const float* yc, int32_t n, int32_t h,
                  int32_t w, float cn_max, int32_t compute_dt, float* dt_io, uint32_t* ws, float* T_next, void* stream);

/* ---- ensemble rollout: b members, each with its own CFL step, clock and stopping time ("Ensemble rollout") ----
 * Device state: T [b][h][w] f32, t [b] f64, t_end [b] f64 (+inf = never stop), steps [b] int32; member m is active iff
 * t[m] < t_end[m].  Every entry point returns MC_EINVAL, launching nothing, for a null pointer (vel_scale alone may be
 * NULL = 1), b <= 0 or b > 65535, h < 5 or w < 5, a uv_stride below h * w, n_steps <= 0 or a cursor outside [0, n_steps].
 * The library allocates nothing.
 * mc_rollout_blocks: workgroups per member of the step kernel, a function of (h, w) alone, so that a member's partial sums
 * do not depend on b; partials holds b * blocks * 8 doubles. */
int32_t mc_rollout_blocks(int32_t h, int32_t w);
/* dx_min[0] = the smallest x[i][j] - x[i][j-1] of the interior (side coordinates 0 / 4 substituted): the grid spacing of
 * mc_adnet_step's CFL step, computed once per grid instead of once per step. */
int mc_rollout_dx_min(const float* xc, int32_t h, int32_t w, float* dx_min, void* stream);
/* Per-member time step: uv_m = max(|s_m u|, |s_m v|) over member m's interior (ws: b x uint32 scratch),
 * dt[m] = fminf(0.5f cn_max dx_min / uv_m, 0.5f dx2 dx2 / (dx2 + dx2)) -- mc_adnet_step's expression, the diffusive limit
 * for a member at rest -- as an f64; flags[m] = 1.  A step that reaches the stopping time, t[m] + dt[m] >= t_end[m], is
 * shortened to dt[m] = t_end[m] - t[m] with flags[m] = 2; an inactive member gets dt[m] = 0, flags[m] = 0. */
int mc_rollout_dt(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* dx_min,
                  const double* t, const double* t_end, int32_t b, int32_t h, int32_t w, float cn_max, uint32_t* ws, double* dt,
                  int32_t* flags, void* stream);
/* mc_adnet_step's stencil with (float)dt[m] per member, wall rows and side columns included; a member with flags[m] = 0 is
 * copied.  The same launch leaves per-workgroup f64 partial sums of the six diagnostics in partials. */
int mc_rollout_step(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* T_prev,
                    const float* raq_scalar, const float* xc, const float* yc, const double* dt, const int32_t* flags, int32_t b,
                    int32_t h, int32_t w, float* T_next, double* partials, void* stream);
/* Reduces the partial sums in a fixed order and writes row cursor[0] of hist [n_steps][b][8] = (t after the step, dt, mean T,
 * v_rms, Nu_bot, Nu_top, min T, max T) of T_next and of the velocity the step used; advances t[m] (set TO t_end[m] when
 * flags[m] = 2) and steps[m] of the members that stepped, then cursor[0].  With the cursor at n_steps the row is dropped. */
int mc_rollout_finalize(const double* partials, const double* dt, const int32_t* flags, const double* t_end, double* t,
                        int32_t* steps, int32_t* cursor, double* hist, int32_t n_steps, int32_t b, int32_t h, int32_t w,
                        void* stream);
/* cursor[0] = row with a one-thread kernel on `stream`. */
int mc_rollout_set_cursor(int32_t* cursor, int32_t row, int32_t n_steps, void* stream);

/* ---- ensemble rollout statistics: depth profiles, their time sums, saves at fixed simulated times ----
 * Both entry points return MC_EINVAL, launching nothing, for a null pointer (vel_scale may be NULL = 1, prof may be NULL),
 * b <= 0 or b > 65535, h < 5 or w < 5, a uv_stride below h * w, capacity <= 0 or T_new == snaps.
 * mc_ensemble_profiles reads the state a step STARTS from: the velocity planes u, v [b][h][w] (batch stride uv_stride,
 * multiplied by vel_scale[m] as mc_rollout_step forms s u, s v: one f32 product) and T [b][h][w], the field that velocity was
 * computed from; dt, flags of mc_rollout_dt, t before mc_rollout_finalize advances it.  prof [b][4][h] f64 = the mean over
 * ALL w columns of row i of (T, (s u)^2, (s v)^2, (s v) T), squares, products and sums in f64: one wave per row, lane l adds
 * columns l, l + 64, ... in order, then the xor tree, then / w.  Time weight of member m: 0 when flags[m] = 0, else
 * t_avg_start[m] <= t[m] ? dt[m] : fmax(0, (t[m] + dt[m]) - t_avg_start[m]).  With a positive weight acc [b][4][h] += weight *
 * prof (one multiply, one add), wsum[m] += weight, nacc[m] += 1; with weight 0 nothing of member m is written but prof. */
int mc_ensemble_profiles(const float* u, const float* v, int64_t uv_stride, const float* vel_scale, const float* T,
                         const double* dt, const int32_t* flags, const double* t, const double* t_avg_start, int32_t b,
                         int32_t h, int32_t w, double* prof, double* acc, double* wsum, int32_t* nacc, void* stream);
/* After mc_rollout_finalize (t is the new clock, T_new [b][h][w] the field just written).  Member m saves iff flags[m] != 0,
 * save_every[m] > 0 and t[m] > next_save[m]; then, with count[m] < capacity, slot[m] = count[m], snap_t[m][slot] = t[m],
 * count[m] += 1 and the plane is copied to snaps [b][capacity][h][w]; with the slots used up slot[m] = -1 and missed[m] += 1;
 * either way next_save[m] = t[m] + save_every[m].  A member that does not save gets slot[m] = -1.  snap_t [b][capacity]. */
int mc_ensemble_snapshot(const float* T_new, const double* t, const int32_t* flags, const double* save_every, double* next_save,
                         int32_t* count, int32_t* missed, int32_t* slot, int32_t capacity, int32_t b, int32_t h, int32_t w,
                         float* snaps, double* snap_t, void* stream);

/* ---- rollout scoring: ensemble members against the snapshots of their simulations ("Rollout scoring") ----
 * One launch BETWEEN mc_rollout_step and mc_rollout_finalize: T_prev, T_next [b][h][w] are the state before / after the step,
 * t is still the old clock; dt, flags of mc_rollout_dt.  truth [b][capacity][h][w] f32 and truth_t [b][capacity] f64 hold the
 * later snapshots of member m's simulation and their simulated times, ascending; only the first min(n_truth[m], capacity)
 * count.  Returns MC_EINVAL, launching nothing, for a null pointer, b <= 0 or b > 65535, h < 5 or w < 5, capacity <= 0 or
 * T_prev == T_next.  The library allocates nothing.
 * Member m with flags[m] = 0 is not touched.  Otherwise t0 = t[m], t1 = flags[m] == 2 ? t_end[m] : t0 + dt[m] (bitwise the
 * clock mc_rollout_finalize stores), and from k = next[m] on, while k < min(n_truth[m], capacity) and tau = truth_t[m][k] <= t1:
 * tau < t0 (a time the clock had passed already) counts in skipped[m] and leaves row k as it is; else row k is scored with
 * theta = t1 > t0 ? (tau - t0) / (t1 - t0) : 0 and counts in scored[m]; k += 1.  Then next[m] = k.  Any number of times may
 * fall into one step.
 * Scoring row k, over ALL h x w cells, every operation in f64: a = (double)T_prev + theta * ((double)T_next - (double)T_prev),
 * b = (double)truth[m][k].  Pass 1: row means A_i, B_i -- lane l adds columns l, l + 64, ... in ascending order, then the xor
 * tree, then / w -- and Abar = (sum_i A_i) / h, Bbar likewise, i ascending.  Pass 2, the same order inside a row and rows added
 * with i ascending: sum|a-b|, max|a-b|, Saa = sum (a-Abar)^2, Sbb = sum (b-Bbar)^2, Sab = sum (a-Abar)(b-Bbar).
 * table [b][capacity][8] row = (tau, theta, mae = sum|a-b| / (h w), max_err, corr = Sab / sqrt(Saa Sbb) (NaN when
 * Saa Sbb == 0), prof_mae = (sum_i |A_i - B_i|) / h, Abar, Bbar); prof [b][capacity][2][h] = (A_i, B_i).  One workgroup per
 * member: a member's rows depend on its own data alone, whatever b is. */
int mc_score_rollout(const float* T_prev, const float* T_next, const double* t, const double* dt, const int32_t* flags,
                     const double* t_end, const float* truth, const double* truth_t, const int32_t* n_truth, int32_t capacity,
                     int32_t b, int32_t h, int32_t w, int32_t* next, int32_t* scored, int32_t* skipped, double* table, double* prof,
                     void* stream);

/* ---- series scoring: a trained Stokes net against the snapshots of a simulation ("Series scoring") ----
 * Store (f32, device): T, u, v [n_snap][h][w] with snapshot stride store_stride (un-scaled, as the files hold them), sim [n_snap]
 * int32 (the snapshot's simulation), prev [n_snap] int32 (its baseline snapshot; outside [0, n_snap) = none), paras [n_sims][3] =
 * (RaQ, FKT, FKP), paras_nd [n_sims][3], inv_scale [n_sims] = 1 / velocity scale.  Work list idx [n_items] int32 and a device
 * cursor (int32): slot k of a step of b slots holds item j = min(cursor + k, n_items - 1) and snapshot s = idx[j]; only slots
 * with cursor + k < n_items write results.  idx[j] and sim[s] are clamped into their ranges before they address anything.
 * Every entry point returns MC_EINVAL, launching nothing, for a null pointer, b <= 0 or b > 65535, h < 3 or w < 3,
 * n_items <= 0, n_snap <= 0, n_sims <= 0, a stride below h * w or a cursor row outside [0, n_items].  The library allocates
 * nothing.
 * mc_series_build_input: out [b][7][h][w], out[k] = mc_ts_build_input's seven channels for T[s] with paras[sim[s]] and
 * paras_nd[sim[s]] (the same f32 expressions: bit-identical to mc_ts_build_input on the gathered arrays); the store is read in
 * place. */
int mc_series_build_input(const float* T, int64_t store_stride, const int32_t* sim, const float* xc, const float* yc,
                          const float* ycc, const float* paras, const float* paras_nd, const int32_t* idx, const int32_t* cursor,
                          int32_t n_items, int32_t n_snap, int32_t n_sims, int32_t b, int32_t h, int32_t w, float* out,
                          void* stream);
/* Row pass.  u_hat, v_hat [b][h][w] with batch stride uv_stride: the network's (scaled) velocities, read in place.  In the scaled
 * space ut = u[s][i][j] * inv_scale[sim[s]] (ONE f32 product), likewise vt, and ub, vb from snapshot prev[s]; every difference,
 * absolute value and sum is f64.  One wave per row (k, i): lane l takes columns l, l + 64, ... in ascending order, then the xor
 * tree.  rows [b][10][h] f64 = sum|ut-u_hat|, sum|vt-v_hat|, sum|ut-ub|, sum|vt-vb| (NaN without a baseline), max|ut|, max|vt|,
 * max|ut-u_hat|, max|vt-v_hat|, and over the interior columns of interior rows sum|div(u_hat,v_hat)|, sum|div(ut,vt)| with
 * div(a,b)[i][j] = 0.5 (a[i][j+1] - a[i][j-1]) + 0.5 (b[i+1][j] - b[i-1][j]) (0 on the first and last row). */
int mc_series_score(const float* u_hat, const float* v_hat, int64_t uv_stride, const float* u, const float* v, int64_t store_stride,
                    const int32_t* sim, const int32_t* prev, const float* inv_scale, const int32_t* idx, const int32_t* cursor,
                    int32_t n_items, int32_t n_snap, int32_t n_sims, int32_t b, int32_t h, int32_t w, double* rows, void* stream);
/* Adds (takes the maximum of) the row results over i ascending and writes table [n_items][10] f64, row j = (mae_u, mae_v, base_u,
 * base_v: sums / (h w); max_u, max_v, maxerr_u, maxerr_v; mass_pred, mass_true: sums / ((h-2)(w-2))), and profile
 * [n_items][2][h] = the row means (/ w) of |ut-u_hat| and |vt-v_hat|; one wave per slot.  Slots past the end of the list write
 * nothing.  Then, in a one-thread launch of its own behind it, cursor[0] = min(cursor[0] + b, n_items). */
int mc_series_score_finalize(const double* rows, const int32_t* idx, int32_t* cursor, int32_t n_items, int32_t n_snap, int32_t b,
                             int32_t h, int32_t w, double* table, double* profile, void* stream);
/* cursor[0] = row with a one-thread kernel on `stream`. */
int mc_series_set_cursor(int32_t* cursor, int32_t row, int32_t n_items, void* stream);

/* ---- spectral layer (SpectralConv2d, pytorch_networks_convae.py:571-635) as a truncated DFT ---- */
/* Only the modes K1 = (0, 1, 2, 3, h-4, h-3, h-2, h-1) x K2 = (0, 1, 2, 3) of rfft2 survive the layer; mode index
 * m = k1i * 4 + k2.  Twiddle tables (f32, built on the host in f64 from integer-reduced arguments):
 * rowtw [h][5][2] = (cos, sin)(2 pi (k y mod h) / h) for k = 0..4, coltw [w][4][2] likewise for k2 = 0..3.
 * Both streaming kernels run one block per (slot, channel block, sample): slot = a chunk of rows x a 256-column strip.
 * mc_spectral_slots: slots per sample (<= 64) for an h x w grid, or -1 when h < 8 or w < 8 (the reference's two corner
 * blocks would overlap or touch the Nyquist column) or the grid needs more than 64 slots of 128 rows.  No atomics. */
int32_t mc_spectral_slots(int32_t h, int32_t w);
/* A(t): x CB8 [n][c8][h][w][8] of the dtype code's type (MC_F32 f32, MC_BF16 bf16, MC_MIX16 f16; a gradient tensor of
 * the mixed mode is passed as MC_BF16) -> per-slot partial mode sums part [n][slots][c8*8][8][4][2] f32. */
int mc_spectral_analyze(const void* x, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, const float* rowtw,
                        const float* coltw, float* part, void* stream);
/* S(C): coef [n][c8*8][8][4][2] f32 -> y CB8 of the dtype code's type, lanes past c exactly zero.  gn_part != NULL: also
 * the GroupNorm partials (sum, sum of squares) per channel of the f32 values before the store rounding,
 * [n][slots][c8*8][2] (the layout mc_gn_finalize_coef reads with tiles = slots). */
int mc_spectral_synthesize(const float* coef, int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, const float* rowtw,
                           const float* coltw, void* y, float* gn_part, void* stream);
/* Mode space, forward: xhat [n][ci8*8][8][4][2] = the slots of part in slot order (kept for the backward pass);
 * coef [n][co8*8][8][4][2] = gamma * sum_i xhat[n][i] Wt[i][o], gamma[k2] = (1, 2, 2, 2) / hw, lanes past c_out zero.
 * w1 / w2: the parameters weights1 / weights2, [c_in][c_out][4][4] interleaved (re, im) f32. */
int mc_spectral_mix_fwd(const float* part, int32_t n, int32_t slots, int32_t c_in, int32_t c_out, int32_t hw, const float* w1,
                        const float* w2, float* xhat, float* coef, void* stream);
/* Mode space, backward: part = A(dy) [n][slots][co8*8][8][4][2]; gbuf [n][co8*8][8][4][2] workspace (G = gamma * the
 * slots in order); dw1 / dw2 ACCUMULATE sum_n conj(xhat[n][i]) G[n][o], the samples in order ((d/dRe, d/dIm) interleaved,
 * what torch keeps in .grad of a complex parameter); dxcoef (may be NULL) [n][ci8*8][8][4][2] = sum_o conj(Wt[i][o]) G[n][o],
 * the coefficients mc_spectral_synthesize turns into the input gradient. */
int mc_spectral_mix_bwd(const float* part, int32_t n, int32_t slots, int32_t c_in, int32_t c_out, int32_t hw, const float* w1,
                        const float* w2, const float* xhat, float* gbuf, float* dw1, float* dw2, float* dxcoef, void* stream);

/* ---- optimizer (torch.optim.Adam, multigpu.py:761-763) --------------------------------------- */
/* One fused multi-tensor step over flat f32 buffers; grad_scale folds the 1/world_size of the
 * data-parallel average; lr is read from device memory so a captured graph can be replayed
 * while MultiStepLR changes it. step_count (device int32) is incremented by the kernel. */
int mc_adam_step_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                      const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                      float grad_scale, int32_t* step_count_dev, void* stream);

/* ---- guarded Adam step: global-norm clipping and non-finite step skipping ---------------------- */
/* Device record of the last mc_grad_guard_eval call.  32 bytes, caller-owned, zeroed once by the caller. */
typedef struct {
  float    norm;        /* || grad_scale * g ||_2 of the last call (f32 rounding of the f64 value; may be +inf; not finite
                           when nonfinite > 0) */
  float    coef;        /* factor applied to the gradient by the last call (1 when not clipping) */
  uint32_t nonfinite;   /* elements of g that were not finite in the last call (saturating) */
  uint32_t skip;        /* 1: the last step was skipped */
  uint32_t skipped;     /* steps skipped since the record was zeroed */
  uint32_t consecutive; /* steps skipped in a row up to and including the last call */
  uint32_t pad[2];
} mc_grad_guard;

/* Number of partial slots the workspace of mc_grad_guard_eval needs (host only, no GPU): one per 256 float4 of the
 * buffer: at least 1, non-decreasing, at most 1024; 0 for numel <= 0. */
int mc_grad_norm_blocks(int64_t numel);
/* Two launches, no atomics, every sum in a fixed order: the record is bit-reproducible.
 *   1. per block, sum g^2 and the count of non-finite g, both accumulated in f64 -> ws[b], ws[blocks + b] (plain stores);
 *   2. one block adds the partials in a fixed order (a tree of fixed shape) and writes the record:
 *        norm64 = grad_scale * sqrt(sum g^2), norm = (float)norm64;
 *        coef   = max_norm > 0 ? min(1, max_norm / (norm64 + 1e-6)) : 1, in f64, stored as f32 (clip_grad_norm_'s formula);
 *                 1 whenever nonfinite > 0;
 *        skip   = skip_nonfinite && nonfinite > 0;
 *      and increments *step_count_dev only when skip == 0 (a skipped step does not advance Adam's t); skipped and
 *      consecutive count the skipped steps, consecutive returns to 0 with the first step taken.
 * ws: [2 * mc_grad_norm_blocks(numel)] doubles; grad 16-byte aligned.  MC_EINVAL (nothing launched) for a null pointer,
 * numel <= 0, a misaligned buffer, max_norm < 0 or NaN.  The library allocates nothing. */
int mc_grad_guard_eval(const float* grad, int64_t numel, float grad_scale, float max_norm, int32_t skip_nonfinite,
                       double* ws, mc_grad_guard* guard, int32_t* step_count_dev, void* stream);
/* mc_adam_step_flat after mc_grad_guard_eval, one launch: stores nothing when guard->skip is set; otherwise mc_adam_step_flat's
 * arithmetic with gs = grad_scale * guard->coef (one f32 product) in place of grad_scale, i.e. the clip acts on the scaled
 * raw gradient and weight_decay * p is added after it (clip_grad_norm_ followed by torch.optim.Adam).  It does NOT touch
 * step_count_dev: mc_grad_guard_eval has. */
int mc_adam_step_flat_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel,
                              const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                              float grad_scale, int32_t* step_count_dev, const mc_grad_guard* guard, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MANTLE_HIP_H */

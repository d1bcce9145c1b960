// Counter-based random bits for dropout and the resident loader's input noise: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
// 1, 2, 3", SC 2011).  Plain integer C++, the same text for the host and the device, so that the CPU tests pin exactly what
// the GroupNorm / activation kernels inline.
//
// The dropout mask is a pure function of (seed, step, layer, logical element): one Philox call serves the 8 channels of the
// CB8 vector v = ((n * C8 + cb) * H + y) * W + x (64 bits) with key = (seed_lo, seed_hi) and counter = (v_lo, v_hi, layer,
// step); channel j takes the 16-bit field (out[j >> 1] >> 16 (j & 1)) & 0xffff and is kept iff field < keep16.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_HD __host__ __device__ inline
#else
#define MC_HD inline
#endif

MC_HD void mc_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;            // Weyl sequence of the key (the bump after round 10 is unused)
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// bit j = channel j of CB8 vector v is kept
MC_HD uint32_t mc_dropout_keep8(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t layer, uint64_t v, uint32_t keep16) {
  uint32_t o[4];
  mc_philox4x32_10((uint32_t)v, (uint32_t)(v >> 32), layer, step, seed_lo, seed_hi, o);
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) bits |= (((o[j >> 1] >> (16 * (j & 1))) & 0xffffu) < keep16 ? 1u : 0u) << j;
  return bits;
}

// Input noise of the resident NewAD loader (reference datasetio.py:604-613 draws U(-1e-5, 1e-5) per interior pixel): a pure
// function of (seed, draw, item, pixel) -- key = (seed_lo, seed_hi), counter = (pixel, item, draw, MC_NOISE_TAG), item = the
// item's index with bit 31 set for the initial-condition store.  With k = out[0] >> 8 and u = (k + 0.5) 2^-24,
// n = (2u - 1) 1e-5 = ((2k + 1 - 2^24) 2^-24) 1e-5: the odd integer has fewer than 25 bits, so the f32 product is one
// rounding of the exact value and |n| < 1e-5 strictly.
#define MC_NOISE_TAG 0x6e6f6973u
#define MC_NOISE_INIT_BIT 0x80000000u
MC_HD float mc_newad_noise(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t item, uint32_t pixel) {
  uint32_t o[4];
  mc_philox4x32_10(pixel, item, draw, MC_NOISE_TAG, seed_lo, seed_hi, o);
  const int32_t odd = (int32_t)(2u * (o[0] >> 8) + 1u) - (1 << 24);
  return ((float)odd * 5.9604644775390625e-8f) * 1e-5f;
}

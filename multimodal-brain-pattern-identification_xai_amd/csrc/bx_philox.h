// The counter-based noise of SmoothGrad, infidelity and sensitivity_max: Philox4x32-10, the fp32 Box-Muller normals of counter word 3 = 0
// and the uniform draws of counter word 3 = 1.  The definition is pinned in include/brainxai.h.  Include only in files built with
// -ffp-contract=off (build.py): every operation after the words rounds on its own.
#pragma once
#include "bx_common.h"

// Philox4x32-10 (Salmon et al., SC 2011; the Random123 generator): ten rounds, the key advanced by the Weyl constants before every round
// but the first.
__device__ __forceinline__ void sg_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// Box-Muller in fp32 on two words: u in (0, 1] and t in [0, 2) are exact, every operation after them is rounded on its own.
__device__ __forceinline__ void sg_normal2(uint32_t wa, uint32_t wb, float& z_even, float& z_odd) {
  const float u = (float)((wa >> 8) + 1u) * 0x1p-24f;
  const float t = (float)(wb >> 8) * 0x1p-23f;
  const float r = sqrtf(-2.f * logf(u));
  z_even = r * cospif(t);
  z_odd = r * sinpif(t);
}
// the four normals of elements 4q .. 4q+3 of draw k of sample b
__device__ __forceinline__ void sg_normal4(uint32_t q, uint32_t k, uint32_t b, uint32_t k0, uint32_t k1, float z[4]) {
  uint32_t w[4];
  sg_philox(q, k, b, 0u, k0, k1, w);
  sg_normal2(w[0], w[1], z[0], z[1]);
  sg_normal2(w[2], w[3], z[2], z[3]);
}
// A uniform draw in [-1, 1) from one word: 24 bits times 2^-23 and the subtraction are both exact in fp32.
__device__ __forceinline__ float sg_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-23f - 1.f; }
// the four uniforms of elements 4q .. 4q+3 of draw k of sample b: counter word 3 is 1, a stream apart from the normals'
__device__ __forceinline__ void sg_uniform4(uint32_t q, uint32_t k, uint32_t b, uint32_t k0, uint32_t k1, float u[4]) {
  uint32_t w[4];
  sg_philox(q, k, b, 1u, k0, k1, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = sg_uniform(w[i]);
}

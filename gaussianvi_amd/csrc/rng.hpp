// Counter-based normal generator of the samplers (gvi_randn / gvi_bt_sample / gvi_ngd_sample), fixed so that a caller can
// restate it (tests/test_sample_host.py does):
//   Philox4x32-10 (Salmon et al., SC'11), key = seed as two 32-bit words, low word first;
//   normal number i of stream `seed`: counter c = i >> 1 in words 0-1 (low first), words 2-3 zero; output words (w0..w3) ->
//   u1 = ((w0 | w1 << 32) >> 11) + 0.5) 2^-53, u2 the same from (w2, w3);  r = sqrt(-2 ln u1),
//   z[2c] = r cos(2 pi u2),  z[2c + 1] = r sin(2 pi u2).
// Draw i depends only on (seed, i): a batch split across calls or ranks gives the same numbers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gvi {

__host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
  }
}

// the two normals of counter c: z[2c] -> z0, z[2c + 1] -> z1
__device__ inline void randn_pair(uint64_t seed, uint64_t c, double& z0, double& z1) {
  uint32_t w[4] = {(uint32_t)c, (uint32_t)(c >> 32), 0u, 0u};
  philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u1 = ((double)((((uint64_t)w[1] << 32) | w[0]) >> 11) + 0.5) * 0x1p-53;
  const double u2 = ((double)((((uint64_t)w[3] << 32) | w[2]) >> 11) + 0.5) * 0x1p-53;
  const double r = sqrt(-2.0 * log(u1));
  double s, co;
  sincos(2.0 * 3.141592653589793 * u2, &s, &co);
  z0 = r * co;
  z1 = r * s;
}

}  // namespace gvi

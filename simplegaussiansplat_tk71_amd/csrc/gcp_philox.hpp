// gcp_philox.hpp — the counter-based random numbers of density control, shared by gcp_densify.hip (split samples) and
// gcp_mcmc.hip (relocation draws, position noise): Philox4x32-10, its mapping to the open unit interval (both consumers
// feed it to the same Box-Muller lines) and the rotation of a quaternion.  Every draw is a pure function of (key,
// counter): the counter's last word tells the consumers apart (0 split children, 1 position noise, 2 relocation draws).
#pragma once
#include <math.h>

#include "gcp_device.hpp"

namespace gcp {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1, c3 = (unsigned)p0, c0 = n0, c2 = n2;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__device__ __forceinline__ float unit_open(unsigned r) { return ((float)r + 0.5f) * 2.3283064365386963e-10f; }  // (r + 0.5) 2^-32, in (0, 1]

// ln u of u = (r + 0.5) 2^-32 to float accuracy over the whole range: the float u has 24 bits, so above 1/2 — where ln u
// goes to 0 and the radius sqrt(-2 ln u) with it — the logarithm is taken from 1 - u = (~r + 0.5) 2^-32, which is exact
// where u is not (r = 2^32 - 1 gives ln u = -1.16e-10, not 0).
__device__ __forceinline__ float log_unit_open(unsigned r) { return r < 0x80000000u ? logf(unit_open(r)) : log1pf(-unit_open(~r)); }

// Row-major rotation of the quaternion (x, y, z, w) / max(|q|, 1e-8): qvec_to_rotmat_batch.
__device__ __forceinline__ void quat_rotation(float x, float y, float z, float w, float r[9]) {
  const float inv = 1.0f / fmaxf(sqrtf(x * x + y * y + z * z + w * w), 1e-8f);
  x *= inv, y *= inv, z *= inv, w *= inv;
  r[0] = 1 - 2 * (y * y + z * z), r[1] = 2 * (x * y - w * z), r[2] = 2 * (x * z + w * y);
  r[3] = 2 * (x * y + w * z), r[4] = 1 - 2 * (x * x + z * z), r[5] = 2 * (y * z - w * x);
  r[6] = 2 * (x * z - w * y), r[7] = 2 * (y * z + w * x), r[8] = 1 - 2 * (x * x + y * y);
}

}  // namespace gcp

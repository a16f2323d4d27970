// Exact x % d for any 32-bit x and a run-time 32-bit d >= 1 by a precomputed reciprocal, shared by the
// host (ethash_host.h, tests/native/ethash_host_main.cpp) and the device (ethash_dev.cuh): the kernels
// reduce by the cache's and the dataset's row counts 32,832 times per header, and a run-time udiv is
// tens of instructions.
//
//   m = floor((2^32 - 1) / d)            once per launch, on the host
//   q = floor(x m / 2^32)                one mul_hi
//   r = x - q d;  if (r >= d) r -= d     one mul_lo, a subtract, a compare and a select
//
// Why one correction is enough: q <= x / d always (m <= 2^32 / d), so r >= 0 and r <= x fits 32 bits.
// From below, for d that is no power of two m = floor(2^32 / d) > 2^32 / d - 1, so
// x m / 2^32 > x / d - x / 2^32 > x / d - 1 and q > x / d - 2, i.e. q >= floor(x / d) - 1.  For d = 2^k,
// k >= 1, m = 2^(32 - k) - 1 and x m / 2^32 = x / 2^k - x / 2^32, the same bound.  For d = 1, m = 2^32 - 1
// gives q = x - 1 (0 for x = 0), r = 1 or 0, corrected to 0.  tests/native/ethash_host_main.cpp drives this
// very function against % at the edges of every quotient step it can reach.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GSV_ETHASH_HD __host__ __device__ __forceinline__
#else
#define GSV_ETHASH_HD inline
#endif

namespace gsv {
namespace ethash {

struct ModRecip {
    uint32_t d;  // the divisor (rows), >= 1
    uint32_t m;  // floor((2^32 - 1) / d)
};

inline ModRecip mod_recip(uint32_t d) { return ModRecip{d, (uint32_t)(0xFFFFFFFFull / d)}; }

GSV_ETHASH_HD uint32_t mod_reduce(uint32_t x, ModRecip r) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t q = __umulhi(x, r.m);
#else
    const uint32_t q = (uint32_t)(((uint64_t)x * r.m) >> 32);
#endif
    const uint32_t t = x - q * r.d;
    return t >= r.d ? t - r.d : t;
}

constexpr uint32_t FNV_PRIME = 0x01000193u;
GSV_ETHASH_HD uint32_t fnv(uint32_t a, uint32_t b) { return a * FNV_PRIME ^ b; }

}  // namespace ethash
}  // namespace gsv

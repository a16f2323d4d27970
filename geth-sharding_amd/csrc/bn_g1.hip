// Batched bn256Add (0x06) and bn256ScalarMul (0x07) on gfx950 (core/vm/contracts.go:274-312): one
// lane per fixed-size record, no prepare step, no tables in memory.  The arithmetic is bn_g1.cuh
// (decode, GLV split, the joint-bit loop on the rescaled curve, one inversion, marshal).
//   k_bn_g1_add      n x 128 B  x1 || y1 || x2 || y2  -> n x 64 B + status
//   k_bn_g1_mul<B>   n x  96 B  x || y || k           -> n x 64 B + status; B = the bit-serial form
// All hold everything in registers: no scratch, no LDS.  The GLV multiplication takes 204 VGPRs (the
// three-entry table, two Jacobian points, a product's operands): two waves per SIMD; the addition
// (132) and the bit-serial form (147) three.
#include "opcount.cuh"
#include "bn_g1.cuh"
#include "gsv_internal.h"

namespace gsv {
namespace bn {

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1))) void k_bn_g1_add(
    const uint8_t* __restrict__ in, uint32_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    status[i] = g1_add_item(out + (size_t)i * 64, in + (size_t)i * 128);
}

template <bool BITSERIAL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1))) void k_bn_g1_mul(
    const uint8_t* __restrict__ in, uint32_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ status) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    status[i] = g1_mul_item<BITSERIAL>(out + (size_t)i * 64, in + (size_t)i * 96);
}

}  // namespace bn

hipError_t launch_bn256_g1_add(const uint8_t* d_in128, uint32_t n, uint8_t* d_out64, uint8_t* d_status,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bn::k_bn_g1_add, dim3((n + 63) / 64), dim3(64), 0, st, d_in128, n, d_out64, d_status);
    return hipGetLastError();
}

hipError_t launch_bn256_g1_mul(const uint8_t* d_in96, uint32_t n, uint8_t* d_out64, uint8_t* d_status,
                               int bitserial, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (bitserial)
        hipLaunchKernelGGL(bn::k_bn_g1_mul<true>, dim3((n + 63) / 64), dim3(64), 0, st, d_in96, n, d_out64,
                           d_status);
    else
        hipLaunchKernelGGL(bn::k_bn_g1_mul<false>, dim3((n + 63) / 64), dim3(64), 0, st, d_in96, n, d_out64,
                           d_status);
    return hipGetLastError();
}

}  // namespace gsv

GSV_OPCOUNT_READER(bn_g1)

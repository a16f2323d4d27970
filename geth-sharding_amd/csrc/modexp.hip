// Batched bigModExp (0x05, core/vm/contracts.go:226-252) on gfx950: one lane per row of base || exp || mod,
// one launch per call.  The arithmetic is modexp_dev.cuh; the kernel is instantiated per width class of the
// modulus (L = 8, 16, 32, 64, 128, 256 limbs), so every limb loop has one bound across a launch.
//   k_modexp<8>   the six numbers of a lane are arrays of its own with constant indices: registers
//   k_modexp<L>   they are the lane's columns of its wave's region of the work buffer (limb i of a wave's 64
//                 lanes is one 256-byte line), but for L <= 64 the accumulator of the products, which is the
//                 lane's column of L x 64 words of LDS (at L = 256 the 64 KiB a wave left one wave per two
//                 SIMDs and ran 1.6 times slower than the work buffer; L = 128 is not measured and goes
//                 with it).  A wave walks the rows in strides of the grid, so the buffer is bounded by the
//                 waves launched (modexp_plan.h work_bytes)
#include "gsv_internal.h"
#include "modexp_dev.cuh"
#include "modexp_plan.h"

namespace gsv {
namespace mdx {

template <int L>
__global__ __launch_bounds__(64) void k_modexp(const uint8_t* __restrict__ in, uint32_t n, uint32_t bl, uint32_t el,
                                               uint32_t ml, uint8_t* __restrict__ out, uint32_t* work) {
    const size_t row = (size_t)bl + el + ml;
    const uint32_t stride = gridDim.x * 64;
    if constexpr (L == 8) {
        uint32_t q[L], t[L], xr[L], acc[L], r2[L], aux[L];
        const Slots w = {q, t, xr, acc, r2, aux};
        for (uint32_t i = blockIdx.x * 64 + threadIdx.x; i < n; i += stride)
            modexp_item<L, 1, true>(in + (size_t)i * row, bl, el, ml, out + (size_t)i * ml, w);
    } else if constexpr (L <= LDS_ACC_MAX_LIMBS) {
        // the accumulator every product rewrites limb by limb stays on the CU: L x 64 words of LDS
        __shared__ uint32_t acc_lds[L * 64];
        uint32_t* p = work + (size_t)blockIdx.x * (64 * 5 * L) + threadIdx.x;
        const Slots w = {p, acc_lds + threadIdx.x, p + 64 * L, p + 2 * 64 * L, p + 3 * 64 * L, p + 4 * 64 * L};
        for (uint32_t i = blockIdx.x * 64 + threadIdx.x; i < n; i += stride)
            modexp_item<L, 64, false>(in + (size_t)i * row, bl, el, ml, out + (size_t)i * ml, w);
    } else {
        uint32_t* p = work + (size_t)blockIdx.x * (64 * 6 * L) + threadIdx.x;
        const Slots w = {p, p + 64 * L, p + 2 * 64 * L, p + 3 * 64 * L, p + 4 * 64 * L, p + 5 * 64 * L};
        for (uint32_t i = blockIdx.x * 64 + threadIdx.x; i < n; i += stride)
            modexp_item<L, 64, false>(in + (size_t)i * row, bl, el, ml, out + (size_t)i * ml, w);
    }
}

template <int L>
static void launch(const uint8_t* d_in, uint32_t n, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* d_out,
                   uint32_t* d_work, hipStream_t st) {
    const uint32_t waves = L == 8 ? (n + 63) / 64 : (uint32_t)waves_for(n);
    hipLaunchKernelGGL(k_modexp<L>, dim3(waves), dim3(64), 0, st, d_in, n, bl, el, ml, d_out, d_work);
}

}  // namespace mdx

hipError_t launch_modexp(const uint8_t* d_in, uint32_t n, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* d_out,
                         uint8_t* d_work, hipStream_t st) {
    if (n == 0 || ml == 0) return hipSuccess;
    uint32_t* w = (uint32_t*)d_work;
    switch (mdx::width_class(ml)) {
        case 0: mdx::launch<8>(d_in, n, bl, el, ml, d_out, w, st); break;
        case 1: mdx::launch<16>(d_in, n, bl, el, ml, d_out, w, st); break;
        case 2: mdx::launch<32>(d_in, n, bl, el, ml, d_out, w, st); break;
        case 3: mdx::launch<64>(d_in, n, bl, el, ml, d_out, w, st); break;
        case 4: mdx::launch<128>(d_in, n, bl, el, ml, d_out, w, st); break;
        case 5: mdx::launch<256>(d_in, n, bl, el, ml, d_out, w, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gsv

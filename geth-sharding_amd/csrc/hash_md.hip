// Batched SHA-256 and RIPEMD-160 over variable-length messages: the sha256hash and ripemd160hash
// precompiles (core/vm/contracts.go:104-133; crypto/sha256.Sum256 and vendor/golang.org/x/crypto/
// ripemd160).  One message per lane; each lane compresses its own 64-byte blocks, which md_block_dev.cuh
// assembles, padding included, from the message where it lies.
#include "gsv_internal.h"
#include "keccak_dev.cuh"
#include "md_block_dev.cuh"
#include "ripemd160_dev.cuh"
#include "sha256_dev.cuh"

namespace gsv {

// Two dwordx4 stores of a 32-byte row when out32 is 16-byte aligned (uniform), bytes otherwise
GSV_DI void store_row32(uint8_t* __restrict__ out32, uint32_t i, const uint32_t (&r)[8]) {
    uint8_t* o = out32 + (size_t)i * 32;
    if (((uintptr_t)out32 & 15u) == 0) {
        uint4* o4 = (uint4*)o;
        o4[0] = make_uint4(r[0], r[1], r[2], r[3]);
        o4[1] = make_uint4(r[4], r[5], r[6], r[7]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
        for (int b = 0; b < 4; b++) o[4 * k + b] = (uint8_t)(r[k] >> (8 * b));
}

// The item this thread hashes: messages are taken in block-count order within each workgroup
// (keccak_dev.cuh wg_bucket_order), so that one long message stalls a wave of long ones, not of short ones
GSV_DI uint32_t md_item(const uint64_t* __restrict__ off, uint32_t n) {
    const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x;
    return wg_bucket_order(i0, i0 < n, i0 < n ? md_block_count(off[i0 + 1] - off[i0]) : 0);
}

// The compression is inlined in the block loop, which is its only call site (one copy of the rounds; the
// out-of-line form of sha256_dev.cuh exists for callers with sixteen sites): DESIGN 3.4d has the
// resource report.
__global__ __launch_bounds__(256) void k_sha256(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                uint32_t n, uint8_t* __restrict__ out32) {
    const uint32_t i = md_item(off, n);
    if (i >= n) return;
    const uint8_t* p = data + off[i];
    const uint64_t len = off[i + 1] - off[i];
    const uint64_t nb = md_block_count(len);
    uint32_t s[8], w[16];
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = SHA256_IV[k];
#pragma unroll 1
    for (uint64_t b = 0; b < nb; b++) {
        md_load_block<true>(w, p, len, b);
        sha256_compress_inline(s, w);
    }
    uint32_t r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = md_bswap(s[k]);  // the digest is the state's words, big-endian
    store_row32(out32, i, r);
}

// The row is the precompile's: common.LeftPadBytes(digest, 32) (contracts.go:132), 12 zero bytes and the
// state's five words, little-endian
__global__ __launch_bounds__(256) void k_ripemd160(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                   uint32_t n, uint8_t* __restrict__ out32) {
    const uint32_t i = md_item(off, n);
    if (i >= n) return;
    const uint8_t* p = data + off[i];
    const uint64_t len = off[i + 1] - off[i];
    const uint64_t nb = md_block_count(len);
    uint32_t h[5], x[16];
    ripemd160_init(h);
#pragma unroll 1
    for (uint64_t b = 0; b < nb; b++) {
        md_load_block<false>(x, p, len, b);
        ripemd160_compress(h, x);
    }
    const uint32_t r[8] = {0u, 0u, 0u, h[0], h[1], h[2], h[3], h[4]};
    store_row32(out32, i, r);
}

hipError_t launch_sha256(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out32, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sha256, dim3((n + 255) / 256), dim3(256), 0, st, data, off, n, out32);
    return hipGetLastError();
}

hipError_t launch_ripemd160(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out32, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ripemd160, dim3((n + 255) / 256), dim3(256), 0, st, data, off, n, out32);
    return hipGetLastError();
}

}  // namespace gsv

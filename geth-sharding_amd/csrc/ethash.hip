// Batched ethash (consensus/ethash): dataset items and hashimotoLight / VerifySeal over a device-resident
// verification cache.
//
//   k_ethash_items   the body of generateDataset (algorithm.go:313-319): one dataset item per lane
//   k_ethash_light   hashimoto (algorithm.go:332-370) with light lookups, TWO adjacent lanes per header.
//                    Lane j of a pair owns mix[16 j .. 16 j + 15] and computes dataset item 2 parent + j:
//                    fnvHash(mix, temp) is element-wise, so that item is exactly the half it needs.  Per
//                    access one word crosses lanes (mix[i % 32], for the next parent); the final compress
//                    leaves four digest words in each lane, exchanged once for the closing Keccak-256.
//                    The dependent chain of row fetches per lane is half of one lane per header's, and a
//                    header keeps twice the loads in flight.
//
// Out of scope here: Header.HashNoNonce() from the header's RLP (callers pass the 32-byte hash;
// gsv_keccak256_batch makes it from the 13-field RLP), the rest of verifyHeader (timestamps, gas limits,
// CalcDifficulty), hashimotoFull with full-DAG storage and the sealer, and cache files on disk.
#include "ethash_dev.cuh"
#include "ethash_host.h"
#include "gsv_internal.h"

namespace gsv {

using namespace ethash;

__global__ __launch_bounds__(256) void k_ethash_items(Cache cache, uint32_t first, uint32_t count,
                                                      uint4* __restrict__ out64) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    uint32_t mix[16];
    dataset_item(mix, cache, first + t);
    uint4* o = out64 + (size_t)t * 4;
    o[0] = make_uint4(mix[0], mix[1], mix[2], mix[3]);
    o[1] = make_uint4(mix[4], mix[5], mix[6], mix[7]);
    o[2] = make_uint4(mix[8], mix[9], mix[10], mix[11]);
    o[3] = make_uint4(mix[12], mix[13], mix[14], mix[15]);
}

// mix[k] for a run-time k, written as a select chain so that no indexed register array goes to scratch.  The
// gfx950 build keeps a copy of mix in LDS instead (64 bytes a lane, 16 KiB a workgroup: four ds_write_b128
// per access and one indexed read), scratch 0
GSV_DI uint32_t mix_word(const uint32_t (&mix)[16], uint32_t k) {
    uint32_t w = mix[0];
#pragma unroll
    for (uint32_t q = 1; q < 16; q++) w = k == q ? mix[q] : w;
    return w;
}

// VERIFY: mix_in / difficulty are read and status written; else mix_out / result_out are written.
template <bool VERIFY>
__global__ __launch_bounds__(256) void k_ethash_light(Cache cache, ModRecip pages, const uint32_t* __restrict__ hash32,
                                                      const uint64_t* __restrict__ nonce, uint32_t n,
                                                      uint8_t* __restrict__ mix_out, uint8_t* __restrict__ result_out,
                                                      const uint8_t* __restrict__ mix_in,
                                                      const uint8_t* __restrict__ difficulty,
                                                      uint8_t* __restrict__ status) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t h = t >> 1;
    if (h >= n) return;  // both lanes of a pair leave together
    const uint32_t j = (uint32_t)(t & 1);
    const int pair_base = (int)((threadIdx.x & 63u) & ~1u);

    uint32_t hw[8], seed[16];
#pragma unroll
    for (int k = 0; k < 8; k++) hw[k] = hash32[h * 8 + k];
    keccak512_40(seed, hw, nonce[h]);
    uint32_t mix[16];
#pragma unroll
    for (int w = 0; w < 16; w++) mix[w] = seed[w];

    // One access per iteration, so that generateDatasetItem is inlined once: the form with mix[i % 32] at
    // compile-time indices (32 accesses per iteration) holds 32 copies of it, 256 VGPRs and one wave per
    // SIMD.  The word that picks the parent is lane (i % 32) / 16's, fetched by both lanes.
#pragma unroll 1
    for (uint32_t i = 0; i < 64; i++) {
        const uint32_t word = (uint32_t)__shfl((int)mix_word(mix, i & 15u), pair_base + (int)((i >> 4) & 1u));
        const uint32_t parent = mod_reduce(fnv(i ^ seed[0], word), pages);
        uint32_t item[16];
        dataset_item(item, cache, 2 * parent + j);
#pragma unroll
        for (int w = 0; w < 16; w++) mix[w] = fnv(mix[w], item[w]);
    }

    // compress: four digest words per lane, words 4 j .. 4 j + 3 of the digest
    uint32_t mine[4], other[4], digest[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        mine[k] = fnv(fnv(fnv(mix[4 * k], mix[4 * k + 1]), mix[4 * k + 2]), mix[4 * k + 3]);
        other[k] = (uint32_t)__shfl_xor((int)mine[k], 1);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        digest[k] = j ? other[k] : mine[k];
        digest[4 + k] = j ? mine[k] : other[k];
    }
    uint32_t result[8];
    keccak256_96(result, seed, digest);
    if (j) return;

    if constexpr (!VERIFY) {
        store_row32(mix_out, h, digest);
        store_row32(result_out, h, result);
    } else {
        // the reference's order (consensus.go:477-499)
        uint32_t d[8], want[8];
        load_row32(d, difficulty, h);
        load_row32(want, mix_in, h);
        uint32_t dnz = 0, diff = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            dnz |= d[k];
            diff |= want[k] ^ digest[k];
        }
        uint8_t st = GSV_ST_OK;
        if (dnz == 0) st = GSV_ST_INVALID_DIFFICULTY;
        else if (diff != 0) st = GSV_ST_INVALID_MIX_DIGEST;
        else if (pow_exceeds_target(result, d)) st = GSV_ST_INVALID_POW;
        status[h] = st;
    }
}

static Cache make_cache_arg(const uint8_t* d_cache, uint64_t cache_bytes) {
    return Cache{(const uint4*)d_cache, mod_recip((uint32_t)(cache_bytes / HASH_BYTES))};
}

hipError_t launch_ethash_items(const uint8_t* d_cache, uint64_t cache_bytes, uint32_t first, uint32_t count,
                               uint8_t* d_out64, hipStream_t st) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ethash_items, dim3((count + 255) / 256), dim3(256), 0, st,
                       make_cache_arg(d_cache, cache_bytes), first, count, (uint4*)d_out64);
    return hipGetLastError();
}

hipError_t launch_ethash_light(const uint8_t* d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                               const uint8_t* d_hash32, const uint64_t* d_nonce, uint32_t n, uint8_t* d_mix32,
                               uint8_t* d_result32, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t threads = 2ull * n;
    hipLaunchKernelGGL(k_ethash_light<false>, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st,
                       make_cache_arg(d_cache, cache_bytes), mod_recip((uint32_t)(dataset_bytes / MIX_BYTES)),
                       (const uint32_t*)d_hash32, d_nonce, n, d_mix32, d_result32, (const uint8_t*)nullptr,
                       (const uint8_t*)nullptr, (uint8_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_ethash_verify(const uint8_t* d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                                const uint8_t* d_hash32, const uint64_t* d_nonce, const uint8_t* d_mix32,
                                const uint8_t* d_difficulty32, uint32_t n, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t threads = 2ull * n;
    hipLaunchKernelGGL(k_ethash_light<true>, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st,
                       make_cache_arg(d_cache, cache_bytes), mod_recip((uint32_t)(dataset_bytes / MIX_BYTES)),
                       (const uint32_t*)d_hash32, d_nonce, n, (uint8_t*)nullptr, (uint8_t*)nullptr, d_mix32,
                       d_difficulty32, d_status);
    return hipGetLastError();
}

}  // namespace gsv

// The pure host functions of the C ABI (include/gsv.h): no context, no device
extern "C" {

uint64_t gsv_ethash_cache_size(uint64_t block) { return gsv::ethash::cache_size(block); }

uint64_t gsv_ethash_dataset_size(uint64_t block) { return gsv::ethash::dataset_size(block); }

int gsv_ethash_seed_hash(uint64_t block, uint8_t* out32) {
    if (!out32) return GSV_E_INVALID_ARG;
    gsv::ethash::seed_hash(block, out32);
    return GSV_SUCCESS;
}

int gsv_ethash_make_cache(const uint8_t* seed32, uint64_t cache_bytes, uint8_t* out) {
    if (!seed32 || !out) return GSV_E_INVALID_ARG;
    return gsv::ethash::make_cache(seed32, cache_bytes, out) ? GSV_SUCCESS : GSV_E_INVALID_ARG;
}

}  // extern "C"

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
//   k_ethash_full    hashimoto with lookups in the device-resident dataset (hashimotoFull, algorithm.go:393-405),
//                    EIGHT adjacent lanes per nonce in the access loop, each reading a quarter of the 128-byte
//                    page (ethash_dev.cuh hashimoto_full); its modes are the plain form, VerifySeal's checks
//                    and the sealer's finish launch
//   k_ethash_search  the same body over n headers x span nonces, the inner loop of mine (sealer.go:97-152): a
//                    winner lowers its header's offset by atomicMin
//
// The header's RLP, Header.HashNoNonce() and the rest of verifyHeader are block_header.hip.  Out of scope: DAG and
// cache files on disk, remote mining / GetWork, and pre-generating the next epoch.
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

// One item per lane, every lane of the workgroup in the body: an item past the batch's end computes the last
// item again and writes nothing.  FM_FULL writes mix_out / result_out; FM_VERIFY reads mix_in / difficulty and
// writes status (the light kernel's checks, in its order); FM_FINISH is the sealer's last launch: item h is
// nonce start[h] + offset[h] when the search left an offset, and it writes nonce_out / mix_out / result_out /
// found, zeros where nothing was found.
enum FullMode { FM_FULL = 0, FM_VERIFY = 1, FM_FINISH = 2 };

template <int MODE>
__global__ __launch_bounds__(FULL_THREADS) void k_ethash_full(Dataset ds, const uint32_t* __restrict__ hash32,
                                                              const uint64_t* __restrict__ nonce, uint32_t n,
                                                              uint8_t* __restrict__ mix_out,
                                                              uint8_t* __restrict__ result_out,
                                                              const uint8_t* __restrict__ mix_in,
                                                              const uint8_t* __restrict__ difficulty,
                                                              uint8_t* __restrict__ status,
                                                              const uint32_t* __restrict__ offset,
                                                              uint64_t* __restrict__ nonce_out) {
    __shared__ FullShared sh;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < n;
    const uint32_t h = live ? t : n - 1;
    uint32_t hw[8];
#pragma unroll
    for (int k = 0; k < 8; k++) hw[k] = hash32[(size_t)h * 8 + k];
    uint64_t nn = nonce[h];
    uint32_t off = 0;
    if constexpr (MODE == FM_FINISH) {
        off = offset[h];
        nn += off;  // mod 2^64, as the reference's nonce++
        // a header with no winner (off = 0xFFFFFFFF) runs the body on that nonce all the same: the body's
        // __syncthreads() takes every lane through it, and its rows are zeroed below
    }
    uint32_t digest[8], result[8];
    hashimoto_full(digest, result, ds, hw, nn, sh);
    if (!live) return;

    if constexpr (MODE == FM_FULL) {
        store_row32(mix_out, h, digest);
        store_row32(result_out, h, result);
    } else if constexpr (MODE == FM_FINISH) {
        const bool found = off != 0xFFFFFFFFu;
        if (!found) {
            nn = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) digest[k] = result[k] = 0;
        }
        // nonce_out is 8-byte aligned (checked on the host); the rows may not be
        nonce_out[h] = nn;
        store_row32(mix_out, h, digest);
        store_row32(result_out, h, result);
        status[h] = found ? 1 : 0;
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

// n headers x span nonces.  A header takes blocks_per_header = ceil(span / 256) consecutive workgroups, so the
// header of a workgroup is uniform; item k of header h is nonce start[h] + k mod 2^64.  A winner (difficulty
// != 0 and result x difficulty < 2^256, pow_exceeds_target) lowers offset[h] to k: the smallest winning k
// whatever the order the workgroups run in.  offset[h] is 0xFFFFFFFF before the launch and span <= 2^32 - 1.
__global__ __launch_bounds__(FULL_THREADS) void k_ethash_search(Dataset ds, const uint32_t* __restrict__ hash32,
                                                                const uint8_t* __restrict__ difficulty,
                                                                const uint64_t* __restrict__ start, uint32_t span,
                                                                uint32_t blocks_per_header,
                                                                uint32_t* __restrict__ offset) {
    __shared__ FullShared sh;
    const uint32_t h = blockIdx.x / blocks_per_header;
    const uint64_t k64 = (uint64_t)(blockIdx.x - h * blocks_per_header) * FULL_THREADS + threadIdx.x;
    const bool live = k64 < span;
    const uint32_t k = live ? (uint32_t)k64 : span - 1;
    uint32_t hw[8];
#pragma unroll
    for (int w = 0; w < 8; w++) hw[w] = hash32[(size_t)h * 8 + w];
    uint32_t digest[8], result[8];
    hashimoto_full(digest, result, ds, hw, start[h] + k, sh);
    uint32_t d[8];
    load_row32(d, difficulty, h);
    uint32_t dnz = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) dnz |= d[w];
    if (live && dnz != 0 && !pow_exceeds_target(result, d)) atomicMin(&offset[h], k);
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

static Dataset make_dataset_arg(const uint8_t* d_dataset, uint64_t dataset_bytes) {
    return Dataset{(const uint4*)d_dataset, mod_recip((uint32_t)(dataset_bytes / MIX_BYTES))};
}

static dim3 full_grid(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + FULL_THREADS - 1) / FULL_THREADS)); }

hipError_t launch_ethash_full(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                              const uint64_t* d_nonce, uint32_t n, uint8_t* d_mix32, uint8_t* d_result32,
                              hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ethash_full<FM_FULL>, full_grid(n), dim3(FULL_THREADS), 0, st,
                       make_dataset_arg(d_dataset, dataset_bytes), (const uint32_t*)d_hash32, d_nonce, n, d_mix32,
                       d_result32, (const uint8_t*)nullptr, (const uint8_t*)nullptr, (uint8_t*)nullptr,
                       (const uint32_t*)nullptr, (uint64_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_ethash_verify_full(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                                     const uint64_t* d_nonce, const uint8_t* d_mix32, const uint8_t* d_difficulty32,
                                     uint32_t n, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ethash_full<FM_VERIFY>, full_grid(n), dim3(FULL_THREADS), 0, st,
                       make_dataset_arg(d_dataset, dataset_bytes), (const uint32_t*)d_hash32, d_nonce, n,
                       (uint8_t*)nullptr, (uint8_t*)nullptr, d_mix32, d_difficulty32, d_status,
                       (const uint32_t*)nullptr, (uint64_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_ethash_search(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                                const uint8_t* d_difficulty32, const uint64_t* d_start, uint32_t n, uint32_t span,
                                uint32_t* d_offset, hipStream_t st) {
    if (n == 0 || span == 0) return hipSuccess;
    const uint32_t bph = (uint32_t)(((uint64_t)span + FULL_THREADS - 1) / FULL_THREADS);
    hipLaunchKernelGGL(k_ethash_search, dim3(n * bph), dim3(FULL_THREADS), 0, st,
                       make_dataset_arg(d_dataset, dataset_bytes), (const uint32_t*)d_hash32, d_difficulty32, d_start,
                       span, bph, d_offset);
    return hipGetLastError();
}

hipError_t launch_ethash_finish(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                                const uint64_t* d_start, const uint32_t* d_offset, uint32_t n, uint64_t* d_nonce_out,
                                uint8_t* d_mix32, uint8_t* d_result32, uint8_t* d_found, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ethash_full<FM_FINISH>, full_grid(n), dim3(FULL_THREADS), 0, st,
                       make_dataset_arg(d_dataset, dataset_bytes), (const uint32_t*)d_hash32, d_start, n, d_mix32,
                       d_result32, (const uint8_t*)nullptr, (const uint8_t*)nullptr, d_found, d_offset, d_nonce_out);
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

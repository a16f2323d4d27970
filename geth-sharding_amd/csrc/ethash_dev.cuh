// consensus/ethash on gfx950: Keccak-512 on keccak_dev.cuh's split-word state, generateDatasetItem
// (algorithm.go:232-261) and the pieces of the hashimoto loop (algorithm.go:332-370) that ethash.hip's
// kernels share.  The cache is the reference's little-endian words, read as four 16-byte loads per row.
#pragma once
#include "ethash_mod.h"
#include "keccak_dev.cuh"

namespace gsv {
namespace ethash {

// Keccak-512 (rate 72, pad 0x01 ... 0x80) of the 64-byte block w, in place: one permutation.  Byte 64 is
// the pad's first and byte 71 its last, both in state word 8.
GSV_DI void keccak512_64(uint32_t w[16]) {
    uint32_t al[25], ah[25];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        al[k] = w[2 * k];
        ah[k] = w[2 * k + 1];
    }
    al[8] = 0x00000001u;
    ah[8] = 0x80000000u;
#pragma unroll
    for (int k = 9; k < 25; k++) al[k] = ah[k] = 0;
    keccakf_split(al, ah);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        w[2 * k] = al[k];
        w[2 * k + 1] = ah[k];
    }
}

// Keccak-512 of the 40-byte seed hash || nonce (little-endian): the pad starts in word 5
GSV_DI void keccak512_40(uint32_t out[16], const uint32_t hash[8], uint64_t nonce) {
    uint32_t al[25], ah[25];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        al[k] = hash[2 * k];
        ah[k] = hash[2 * k + 1];
    }
    al[4] = (uint32_t)nonce;
    ah[4] = (uint32_t)(nonce >> 32);
    al[5] = 0x00000001u;
    ah[5] = 0;
#pragma unroll
    for (int k = 6; k < 25; k++) al[k] = ah[k] = 0;
    ah[8] = 0x80000000u;
    keccakf_split(al, ah);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        out[2 * k] = al[k];
        out[2 * k + 1] = ah[k];
    }
}

// Keccak-256 (rate 136) of the 96 bytes seed || digest: one permutation, of which only the digest's four
// words are read (keccakf_split_digest)
GSV_DI void keccak256_96(uint32_t out[8], const uint32_t seed[16], const uint32_t digest[8]) {
    uint32_t al[25], ah[25];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        al[k] = seed[2 * k];
        ah[k] = seed[2 * k + 1];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        al[8 + k] = digest[2 * k];
        ah[8 + k] = digest[2 * k + 1];
    }
    al[12] = 0x00000001u;
    ah[12] = 0;
#pragma unroll
    for (int k = 13; k < 25; k++) al[k] = ah[k] = 0;
    ah[16] = 0x80000000u;
    keccakf_split_digest(al, ah);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        out[2 * k] = al[k];
        out[2 * k + 1] = ah[k];
    }
}

// what a launch knows of the cache: its rows as uint4 quarters and the reciprocal of the row count
struct Cache {
    const uint4* rows;
    ModRecip rr;
};

GSV_DI void load_row(uint32_t r[16], const Cache& c, uint32_t row) {
    const uint4* p = c.rows + (size_t)row * 4;
    const uint4 a = p[0], b = p[1], d = p[2], e = p[3];
    r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w;
    r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w;
    r[8] = d.x, r[9] = d.y, r[10] = d.z, r[11] = d.w;
    r[12] = e.x, r[13] = e.y, r[14] = e.z, r[15] = e.w;
}

// generateDatasetItem: Keccak-512, 256 parents (each a reduction, a 64-byte row and 16 fnv steps, every one
// depending on the one before), Keccak-512.  The parent loop runs 16 rounds per iteration so that
// mix[i % 16] is a register, not an indexed array.
GSV_DI void dataset_item(uint32_t mix[16], const Cache& c, uint32_t index) {
    load_row(mix, c, mod_reduce(index, c.rr));
    mix[0] ^= index;
    keccak512_64(mix);
#pragma unroll 1
    for (uint32_t i0 = 0; i0 < 256; i0 += 16) {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint32_t parent = mod_reduce(fnv(index ^ (i0 + k), mix[k]), c.rr);
            uint32_t row[16];
            load_row(row, c, parent);
#pragma unroll
            for (int w = 0; w < 16; w++) mix[w] = fnv(mix[w], row[w]);
        }
    }
    keccak512_64(mix);
}

// a 32-byte row of eight little-endian words: two 16-byte stores when the base is 16-byte aligned
// (uniform), bytes otherwise
GSV_DI void store_row32(uint8_t* __restrict__ base, size_t i, const uint32_t (&r)[8]) {
    uint8_t* o = base + i * 32;
    if (((uintptr_t)base & 15u) == 0) {
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

// a 32-byte row of any alignment as eight little-endian words
GSV_DI void load_row32(uint32_t (&r)[8], const uint8_t* __restrict__ base, size_t i) {
    const uint8_t* p = base + i * 32;
#pragma unroll
    for (int k = 0; k < 8; k++)
        r[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 |
               (uint32_t)p[4 * k + 3] << 24;
}

// consensus.go:496-498 without the division: result > floor((2^256 - 1) / difficulty) exactly when the
// 512-bit product result x difficulty has a non-zero high half (r <= floor(M / d) <=> r d <= M for
// integers).  Both are 32 bytes big-endian, given as the little-endian words of their byte strings;
// limb j (least significant first) is bswap of word 7 - j.
GSV_DI bool pow_exceeds_target(const uint32_t (&result)[8], const uint32_t (&difficulty)[8]) {
    uint32_t a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = __builtin_bswap32(result[7 - j]);
        b[j] = __builtin_bswap32(difficulty[7 - j]);
    }
    // column sums of the schoolbook product, least significant first; only the carry into column 8 and
    // the columns above it decide
    uint64_t carry = 0;
    uint32_t high = 0;
#pragma unroll
    for (int col = 0; col < 15; col++) {
        uint64_t lo = carry & 0xFFFFFFFFull, hi = carry >> 32;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int j = col - i;
            if (j < 0 || j > 7) continue;
            const uint64_t p = (uint64_t)a[i] * b[j];
            lo += p & 0xFFFFFFFFull;
            hi += p >> 32;
        }
        hi += lo >> 32;
        if (col >= 8) high |= (uint32_t)lo;
        carry = hi;
    }
    return (high | (uint32_t)carry | (uint32_t)(carry >> 32)) != 0;
}

// ---- hashimoto over the resident dataset (algorithm.go:393-405), shared by k_ethash_full, k_ethash_search and
// the sealer's finish launch.  Keccak is one nonce per lane; the access loop is EIGHT adjacent lanes per nonce:
// lane l of a group holds mix words 4l .. 4l + 3 and reads quarter l of the 128-byte page, so the group reads
// one whole line per access and a wave instruction eight of them.  A group walks its eight nonces FULL_NI at a
// time (independent chains, FULL_NI pages in flight per group).  Seeds go to the group and digest words come
// back through LDS (96 bytes a lane); every lane of the workgroup must call this (two __syncthreads()).
constexpr int FULL_THREADS = 256;
constexpr int FULL_NI = 4;  // nonces a group interleaves; divides 8

struct Dataset {
    const uint4* pages;  // 128-byte aligned: a page is one cache line, eight uint4
    ModRecip rr;         // of the page count, dataset_bytes / 128 (at most 2^31)
};

struct FullShared {
    uint4 seed[FULL_THREADS * 4];
    uint32_t digest[FULL_THREADS * 8];
};

template <int K>
GSV_DI uint32_t comp(const uint4& v) {
    if constexpr (K == 0) return v.x;
    else if constexpr (K == 1) return v.y;
    else if constexpr (K == 2) return v.z;
    else return v.w;
}

// accesses i0 + K .. i0 + 31 of FULL_NI nonces, K a compile-time index: mix[(i0 + K) % 32] is component K % 4
// of lane K / 4's register
template <int K>
GSV_DI void full_accesses(uint4 (&mix)[FULL_NI], const uint32_t (&head)[FULL_NI], const Dataset& ds, uint32_t i0,
                          uint32_t l, int group_lane) {
    if constexpr (K < 32) {
        uint4 page[FULL_NI];
        const uint4* at[FULL_NI];
#pragma unroll
        for (int c = 0; c < FULL_NI; c++) {
            const uint32_t word = (uint32_t)__shfl((int)comp<K % 4>(mix[c]), group_lane + K / 4);
            const uint32_t parent = mod_reduce(fnv((i0 + K) ^ head[c], word), ds.rr);
            at[c] = ds.pages + ((size_t)parent * 8 + l);
        }
        // The FULL_NI loads issue back to back, and nothing crosses the two fences: left to itself the
        // scheduler sinks each load to its own fnv, runs one chain ahead of the others and waits for every
        // load alone (s_waitcnt vmcnt(0) after each: one line in flight per group)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < FULL_NI; c++) page[c] = *at[c];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < FULL_NI; c++) {
            mix[c].x = fnv(mix[c].x, page[c].x);
            mix[c].y = fnv(mix[c].y, page[c].y);
            mix[c].z = fnv(mix[c].z, page[c].z);
            mix[c].w = fnv(mix[c].w, page[c].w);
        }
        full_accesses<K + 1>(mix, head, ds, i0, l, group_lane);
    }
}

GSV_DI void hashimoto_full(uint32_t (&digest)[8], uint32_t (&result)[8], const Dataset& ds, const uint32_t (&hw)[8],
                           uint64_t nonce, FullShared& sh) {
    const uint32_t tid = threadIdx.x, l = tid & 7u, group = tid & ~7u;
    const int group_lane = (int)((tid & 63u) & ~7u);
    uint32_t seed[16];
    keccak512_40(seed, hw, nonce);
#pragma unroll
    for (int q = 0; q < 4; q++)
        sh.seed[tid * 4 + q] = make_uint4(seed[4 * q], seed[4 * q + 1], seed[4 * q + 2], seed[4 * q + 3]);
    __syncthreads();
#pragma unroll 1
    for (uint32_t s0 = 0; s0 < 8; s0 += FULL_NI) {
        uint4 mix[FULL_NI];
        uint32_t head[FULL_NI];
#pragma unroll
        for (int c = 0; c < FULL_NI; c++) {
            const uint32_t src = (group + s0 + c) * 4;
            mix[c] = sh.seed[src + (l & 3u)];  // mix = seed || seed: words 4l .. 4l + 3 are the seed's 4 (l % 4) ..
            head[c] = sh.seed[src].x;
        }
#pragma unroll 1
        for (uint32_t i0 = 0; i0 < 64; i0 += 32) full_accesses<0>(mix, head, ds, i0, l, group_lane);
#pragma unroll
        for (int c = 0; c < FULL_NI; c++)
            sh.digest[(group + s0 + c) * 8 + l] = fnv(fnv(fnv(mix[c].x, mix[c].y), mix[c].z), mix[c].w);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = sh.seed[tid * 4 + q];
        seed[4 * q] = v.x, seed[4 * q + 1] = v.y, seed[4 * q + 2] = v.z, seed[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) digest[k] = sh.digest[tid * 8 + k];
    keccak256_96(result, seed, digest);
}

}  // namespace ethash
}  // namespace gsv

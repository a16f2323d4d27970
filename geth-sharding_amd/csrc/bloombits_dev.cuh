// Device helpers of bloombits.hip: the 8 x 8 bit transposition of the generator, the wave-wide sums of the codec
// and the expansion, and the rule evaluation the matcher and bloomFilter share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bloombits_host.h"

#ifndef GSV_DI
#define GSV_DI __device__ __forceinline__
#endif

namespace gsv {
namespace bb {

// The 8 x 8 bit matrix in x (bit 8 r + c = row r, column c) transposed about its main diagonal: three rounds of
// swaps, of 1 x 1, 2 x 2 and 4 x 4 blocks.
GSV_DI uint64_t transpose8(uint64_t x) {
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
    x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
    x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
    x ^= t ^ (t << 28);
    return x;
}

// inclusive sum over the lanes of a wave of 64
GSV_DI uint32_t wave_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
GSV_DI uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
GSV_DI uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        v += (uint64_t)hi << 32 | lo;
    }
    return v;
}
GSV_DI uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

// bytes [4 w, 4 w + 4) of a row of `bytes` bytes as a little-endian word, zeros past the row's end; `fast`: the row
// is 4-byte aligned and a whole number of words
GSV_DI uint32_t row_word(const uint8_t* __restrict__ row, uint32_t w, uint32_t bytes, bool fast) {
    if (fast) return ((const uint32_t*)row)[w];
    uint32_t v = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
        if (4 * w + b < bytes) v |= (uint32_t)row[4 * w + b] << (8 * b);
    return v;
}
GSV_DI void row_word_store(uint8_t* __restrict__ row, uint32_t w, uint32_t bytes, bool fast, uint32_t v) {
    if (fast) {
        ((uint32_t*)row)[w] = v;
        return;
    }
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
        if (4 * w + b < bytes) row[4 * w + b] = (uint8_t)(v >> (8 * b));
}

// The filter system of one query over a test of one bit number: all ones (matcher.go:238), per rule the OR over its
// clauses of the AND of the clause's three tests (:337-359; no clause: zeros, :361-363), ANDed over the rules
// (:364-366).  test(bit) returns a word of 32 verdicts (the matcher: 32 blocks of a row) or of one (bloomFilter:
// all ones or zero).  Entries of the tables past n_rules / n_clauses are clamped.
template <typename Test>
GSV_DI uint32_t eval_query(const uint16_t* __restrict__ clauses, uint32_t n_clauses,
                           const uint32_t* __restrict__ rule_off, uint32_t n_rules, uint32_t r0, uint32_t r1,
                           Test test) {
    uint32_t acc = 0xFFFFFFFFu;
    r1 = min(r1, n_rules);
#pragma unroll 1
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t c0 = rule_off[r], c1 = min(rule_off[r + 1], n_clauses);
        uint32_t any = 0;
#pragma unroll 1
        for (uint32_t c = c0; c < c1; c++)
            any |= test(clauses[3 * c] & 2047u) & test(clauses[3 * c + 1] & 2047u) & test(clauses[3 * c + 2] & 2047u);
        acc &= any;
    }
    return acc;
}

// of the 8 blocks first .. first + 7 (byte mask 1 << (7 - k) for block first + k) those inside [begin, end]
GSV_DI uint32_t range_mask8(uint64_t first, uint64_t begin, uint64_t end) {
    if (end < first || begin > first + 7 || begin > end) return 0;
    const uint32_t lo = begin > first ? (uint32_t)(begin - first) : 0u;
    const uint32_t hi = end < first + 7 ? (uint32_t)(end - first) : 7u;
    return (0xFFu >> lo) & (0xFFu << (7 - hi)) & 0xFFu;
}

}  // namespace bb
}  // namespace gsv

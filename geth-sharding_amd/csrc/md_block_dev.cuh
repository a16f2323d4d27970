// The block loader of the Merkle-Damgard hashes (SHA-256, RIPEMD-160): the 16 words of 64-byte block b of
// the padded form of a message of `len` bytes at any byte address.  As keccak.hip's load_block does, it reads
// aligned dwords from the block's address rounded down to 4 and realigns them with v_alignbyte_b32: at
// most 17 loads a block instead of 64 byte loads.  A dword is read only if it holds a byte of the
// message, so nothing is read past the end of the batch (nor before its start); the bytes of such a dword
// that belong to a neighbour are masked away.  The padding is written in place: 0x80 after the last
// byte, zeros, and the 64-bit bit length in the last block's words 14 and 15, big-endian for SHA-256
// and little-endian for RIPEMD-160; a message with len % 64 >= 56 gets a second padding block.
// SHA-256's words are big-endian: one v_perm_b32 each.
// The padding logic is plain C++; a host compiler gets byte-wise forms of the two device primitives
// (tests/native/md_hash_host.cpp), of which the dword read touches exactly the valid bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MD_FN __device__ __forceinline__
#else
#define MD_FN static inline
#endif

namespace gsv {

// blocks of the padded message: len bytes, 0x80, and 8 bytes of length, rounded up to 64
MD_FN uint64_t md_block_count(uint64_t len) { return (len + 72) >> 6; }

#if defined(__HIPCC__)
// dword j of q when it holds a byte of [sh, need) (byte offsets from q), else 0
MD_FN uint32_t md_ld_dword(const uint32_t* q, int j, uint32_t sh, uint32_t need) { return 4u * j < need ? q[j] : 0u; }
// bytes sh .. sh + 3 of the little-endian pair (hi:lo)
MD_FN uint32_t md_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
MD_FN uint32_t md_bswap(uint32_t x) { return __builtin_amdgcn_perm(0u, x, 0x00010203u); }
#else
MD_FN uint32_t md_ld_dword(const uint32_t* q, int j, uint32_t sh, uint32_t need) {
    const uint8_t* q8 = (const uint8_t*)q;
    uint32_t v = 0;
    for (uint32_t t = 0; t < 4; t++) {
        const uint32_t at = 4u * j + t;
        if (at >= sh && at < need) v |= (uint32_t)q8[at] << (8 * t);
    }
    return v;
}
MD_FN uint32_t md_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
    return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo;
}
MD_FN uint32_t md_bswap(uint32_t x) { return __builtin_bswap32(x); }
#endif

// w = the little-endian words of the 64 bytes at p, of which the first `avail` (0 .. 64) are the message's;
// the rest come out as zero and are not read
MD_FN void md_load_words(uint32_t (&w)[16], const uint8_t* p, uint32_t avail) {
    const uint32_t* q = (const uint32_t*)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t need = avail ? sh + avail : 0u;  // bytes from q
    uint32_t d[17];
#pragma unroll
    for (int j = 0; j < 17; j++) d[j] = md_ld_dword(q, j, sh, need);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        uint32_t v = md_alignbyte(d[k + 1], d[k], sh);
        const int32_t valid = (int32_t)avail - 4 * k;
        if (valid < 4) v = valid <= 0 ? 0u : v & ((1u << (8 * valid)) - 1u);
        w[k] = v;
    }
}

// Block b (< md_block_count(len)) of the padded message at p.  BE: SHA-256's byte order (big-endian words
// and length); otherwise RIPEMD-160's (little-endian both).
template <bool BE>
MD_FN void md_load_block(uint32_t (&w)[16], const uint8_t* p, uint64_t len, uint64_t b) {
    const uint64_t at = b << 6;
    if (len >= at + 64) {  // a whole block of message: every predicate above folds but dword 16's
        md_load_words(w, p + at, 64u);
    } else {
        const uint32_t avail = len > at ? (uint32_t)(len - at) : 0u;
        md_load_words(w, p + at, avail);
        if (len >= at) {  // the 0x80 byte falls in this block
#pragma unroll
            for (int k = 0; k < 16; k++)
                if ((avail >> 2) == (uint32_t)k) w[k] |= 0x80u << (8 * (avail & 3u));
        }
    }
    if (BE) {
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = md_bswap(w[k]);
    }
    if (b + 1 == md_block_count(len)) {
        const uint64_t bits = len << 3;  // in 64 bits: a message of 2^29 bytes or more has a high word
        w[14] = BE ? (uint32_t)(bits >> 32) : (uint32_t)bits;
        w[15] = BE ? (uint32_t)bits : (uint32_t)(bits >> 32);
    }
}

}  // namespace gsv

// Consensus receipts on gfx950: the strict RLP decode of rlp.DecodeBytes into types.Receipt (receiptRLP,
// core/types/receipt.go:67-128; rlpLog, core/types/log.go:65-95; rlp/decode.go), the 2,048-bit logs bloom
// (bloom9 / LogsBloom / CreateBloom, core/types/bloom9.go:94-127) and the pieces receipt.hip's kernels share.
// The string rules (rlp_string, rlp_fixed) are block_header_dev.cuh's; the list head is the same rule for 0xC0.
// Plain C++.
#pragma once
#include "block_header_dev.cuh"
#include "receipt_host.h"

namespace gsv {
namespace rc {

using bh::rlp_fixed;
using bh::rlp_string;

// One list item of a list that ends at `end` (readKind, rlp/decode.go:920-984): its payload is p[pos .. lend)
// afterwards.  false: no element left, a string where a list belongs, a length that reaches past the enclosing
// list, a long form for a short length or a leading zero in a length.
GSV_DI bool rlp_list(const uint8_t* __restrict__ p, uint32_t& pos, uint32_t end, uint32_t& lend) {
    if (pos >= end) return false;
    const uint32_t b = p[pos];
    if (b < 0xC0u) return false;
    uint32_t start = pos + 1, size = b - 0xC0u;
    if (b > 0xF7u) {
        const uint32_t ll = b - 0xF7u;
        if (ll > 4 || ll > end - start) return false;
        size = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < ll; k++) size = size << 8 | p[start + k];
        if (p[start] == 0 || size < 56) return false;
        start += ll;
    }
    if (size > end - start) return false;
    pos = start;
    lend = start + size;
    return true;
}

// A bloom item for k_receipt_bloom: where its RLP head byte (0x94 or 0xa0) lies, counted from the first
// receipt's first byte, and which of the two it is.  An item takes at least 21 bytes of RLP, so at / 21 is a
// slot of its own in a table of vals_bytes / 21 + 1 entries (receipt_host.h: SLOT_BYTES, slot_count).
constexpr uint64_t D_VALID = 1ull << 63, D_TOPIC = 1ull << 62;
constexpr uint32_t D_DELTA_SHIFT = 32;  // at % 21 above the receipt's index

GSV_DI uint64_t item_desc(uint64_t at, bool topic, uint32_t receipt) {
    return D_VALID | (topic ? D_TOPIC : 0) | (at % SLOT_BYTES) << D_DELTA_SHIFT | receipt;
}

// rlp.DecodeBytes(item, &types.Receipt{}) over p[0 .. len): GSV_ST_OK, GSV_ST_BAD_RLP for whatever the
// reference's decoder refuses, GSV_ST_RECEIPT_STATUS where setStatus does (receipt.go:116-128).  The order is
// the reference's: the struct decodes first (receipt.go:106), then the status field is judged (:109), and
// DecodeBytes looks for bytes behind the list last (rlp/decode.go:142-144).  gas = CumulativeGasUsed of a
// receipt that decodes.  On its way it writes one descriptor per log address and topic into the zero-filled
// table (base = the receipt's first byte counted from the first receipt's).  A receipt that fails must leave
// none: run it again with CLEAR, which walks the same bytes to the same verdict and writes zeros over the same
// slots.  No byte outside p[0 .. len) is read.
template <bool CLEAR>
GSV_DI uint32_t decode_receipt(const uint8_t* __restrict__ p, uint32_t len, uint64_t& gas,
                               uint64_t* __restrict__ desc, uint64_t base, uint32_t receipt) {
    gas = 0;
    uint32_t pos = 0, end, off, n, slen;
    if (!rlp_list(p, pos, len, end)) return GSV_ST_BAD_RLP;  // empty, a string, a size past the input
    // PostStateOrStatus []byte, CumulativeGasUsed uint64 (decodeUint :239-247), Bloom [256]byte
    if (!rlp_string(p, pos, end, off, slen)) return GSV_ST_BAD_RLP;
    const bool status_ok = slen == 0 || slen == 32 || (slen == 1 && p[off] == 0x01);
    if (!rlp_string(p, pos, end, off, n) || (n && p[off] == 0) || n > 8) return GSV_ST_BAD_RLP;
    const uint64_t g = bh::read_be_u64(p + off, n);
    if (!rlp_fixed<256>(p, pos, end, off)) return GSV_ST_BAD_RLP;
    // Logs []*Log: any number of rlpLog{Address [20]byte, Topics [][32]byte, Data []byte}
    uint32_t lend;
    if (!rlp_list(p, pos, end, lend)) return GSV_ST_BAD_RLP;
    if (lend != end) return GSV_ST_BAD_RLP;  // a fifth element
#pragma unroll 1
    while (pos < lend) {
        uint32_t gend, tend;
        if (!rlp_list(p, pos, lend, gend)) return GSV_ST_BAD_RLP;
        uint32_t at = pos;
        if (!rlp_fixed<20>(p, pos, gend, off)) return GSV_ST_BAD_RLP;
        desc[(base + at) / SLOT_BYTES] = CLEAR ? 0 : item_desc(base + at, false, receipt);
        if (!rlp_list(p, pos, gend, tend)) return GSV_ST_BAD_RLP;
#pragma unroll 1
        while (pos < tend) {
            at = pos;
            if (!rlp_fixed<32>(p, pos, tend, off)) return GSV_ST_BAD_RLP;
            desc[(base + at) / SLOT_BYTES] = CLEAR ? 0 : item_desc(base + at, true, receipt);
        }
        if (!rlp_string(p, pos, gend, off, n)) return GSV_ST_BAD_RLP;
        if (pos != gend) return GSV_ST_BAD_RLP;  // a fourth element
    }
    if (!status_ok) return GSV_ST_RECEIPT_STATUS;
    if (end != len) return GSV_ST_BAD_RLP;  // bytes behind the list
    gas = g;
    return GSV_ST_OK;
}

// The 20 or 32 bytes at p as the first words of one padded rate block: a[0 .. 4] (a[5 .. 15] are zero and
// a[16] carries the 0x80).  Reads the aligned dwords that hold a byte of p[0 .. len) and no other.
GSV_DI void load_item(uint64_t (&a)[5], const uint8_t* __restrict__ p, bool topic) {
    const uint32_t* q = (const uint32_t*)((uintptr_t)p & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t need = sh + (topic ? 32u : 20u);
    uint32_t d[9];
#pragma unroll
    for (int j = 0; j < 9; j++) d[j] = (4u * j < need) ? q[j] : 0u;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    a[0] = (uint64_t)w[0] | (uint64_t)w[1] << 32;
    a[1] = (uint64_t)w[2] | (uint64_t)w[3] << 32;
    // an address ends in the middle of word 2: the 0x01 of the padding follows it
    a[2] = (uint64_t)w[4] | (topic ? (uint64_t)w[5] << 32 : 0x01ull << 32);
    a[3] = topic ? (uint64_t)w[6] | (uint64_t)w[7] << 32 : 0;
    a[4] = topic ? 0x01ull : 0;
}

// calcBloomIndexes: bit k of bloom9 is the low 11 bits of the big-endian pair of digest bytes 2k, 2k + 1
// (bloom9.go:120-124); h = the digest's first 8 bytes as a little-endian word
GSV_DI uint32_t bloom_index(uint64_t h, int k) {
    const uint32_t hi = (uint32_t)(h >> (16 * k)) & 0xFFu, lo = (uint32_t)(h >> (16 * k + 8)) & 0xFFu;
    return (hi << 8 | lo) & 2047u;
}

// Keccak-256 of one bloom item, the first 8 digest bytes
GSV_DI uint64_t item_digest(const uint8_t* __restrict__ p, bool topic) {
    uint64_t a[25], w[5];
    load_item(w, p, topic);
#pragma unroll
    for (int k = 0; k < 25; k++) a[k] = k < 5 ? w[k] : 0;
    a[16] = 0x8000000000000000ULL;
    keccakf_digest(a);
    return a[0];
}

// ORs bit b of a 2,048-bit bloom into the 256-byte row at `row`: byte 255 - b / 8 under mask 1 << (b % 8), the
// big.Int layout (core/bloombits/generator.go:64-70).  The row has any byte alignment: the atomic goes to the
// aligned dword that holds the byte and ORs zeros into that dword's other three bytes.
GSV_DI void bloom_or_bit(uint8_t* __restrict__ row, uint32_t b) {
    const uintptr_t at = (uintptr_t)(row + (255u - (b >> 3)));
    atomicOr((uint32_t*)(at & ~(uintptr_t)3), (1u << (b & 7u)) << (8u * (uint32_t)(at & 3u)));
}

}  // namespace rc
}  // namespace gsv

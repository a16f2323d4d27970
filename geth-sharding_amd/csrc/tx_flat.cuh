// A transaction's RLP read from contiguous memory by one lane: the byte / dword view, the txdata item
// decoder and the byte stream [list header][six-item segment][tail] that types.SignTx hashes twice
// (the sighash preimage, then the signed encoding).  csrc/txsign.hip is the user.
//
// The decode rules are rlp/decode.go's for txdata exactly as csrc/tx_host.hip (tx_prepare) and
// csrc/notary.hip (k_notary_tx) state them; tests/tx_rules_model.py is the independent model all three
// are tested against.  notary.hip reads through the blob codec's chunk map and keeps its own copy of the
// decoder: its kernel's instruction count and registers are pinned, so nothing is shared by template.
#pragma once
#include "keccak_dev.cuh"

namespace gsv {

GSV_DI uint32_t ldg32(uintptr_t a) { return *(const __attribute__((address_space(1))) uint32_t*)a; }

// One item of a flat batch: bytes base[0 .. len).
struct FlatView {
    const uint8_t* base;
    uintptr_t hi;  // the last 4-byte-aligned dword holding a byte of the item
    GSV_DI FlatView(const uint8_t* b, uint32_t len) : base(b), hi(((uintptr_t)b + (len ? len - 1u : 0u)) & ~(uintptr_t)3) {}
    GSV_DI uint8_t at(uint32_t k) const { return base[k]; }
    // Bytes k .. k+3 as one little-endian word (byte k lowest): two aligned dwords, realigned.  Past the
    // item's end the bytes are unspecified (callers mask them); the second dword is clamped to `hi`, so
    // every dword read holds a byte of the item and none lies in another page than such a byte.
    GSV_DI uint32_t dword(uint32_t k) const {
        uintptr_t a = (uintptr_t)base + k;
        uintptr_t A = a & ~(uintptr_t)3;
        uint32_t x0 = ldg32(A <= hi ? A : hi), x1 = ldg32(A + 4 <= hi ? A + 4 : hi);
        return __builtin_amdgcn_alignbyte(x1, x0, (uint32_t)a & 3u);
    }
};

struct FItem {
    uint32_t off, n;  // payload offset / length within the transaction
    uint32_t start;   // item start (header) offset
    bool list;
};

// one RLP item at [p, p + len) of the transaction; consumed bytes or 0 on error (canonical single bytes
// and sizes, rlp/decode.go; the same rules as tx_host.hip rlp_item)
GSV_DI uint32_t flat_rlp_item(const FlatView& b, uint32_t p, uint32_t len, FItem& it) {
    if (len == 0) return 0;
    uint32_t b0 = b.at(p);
    it.start = p;
    if (b0 < 0x80) {
        it.off = p;
        it.n = 1;
        it.list = false;
        return 1;
    }
    if (b0 < 0xb8) {
        uint32_t n = b0 - 0x80;
        if (1 + n > len) return 0;
        if (n == 1 && b.at(p + 1) < 0x80) return 0;
        it.off = p + 1;
        it.n = n;
        it.list = false;
        return 1 + n;
    }
    if (b0 < 0xc0 || b0 >= 0xf8) {  // long string / long list
        bool list = b0 >= 0xf8;
        uint32_t nb = list ? b0 - 0xf7 : b0 - 0xb7;
        if (nb > 8 || 1 + nb > len || b.at(p + 1) == 0) return 0;
        uint64_t n = 0;
        for (uint32_t i = 0; i < nb; i++) n = (n << 8) | b.at(p + 1 + i);
        if (n < 56 || n > (uint64_t)(len - 1 - nb)) return 0;
        it.off = p + 1 + nb;
        it.n = (uint32_t)n;
        it.list = list;
        return 1 + nb + (uint32_t)n;
    }
    uint32_t n = b0 - 0xc0;  // short list
    if (1 + n > len) return 0;
    it.off = p + 1;
    it.n = n;
    it.list = true;
    return 1 + n;
}
// uint64 (Stream.uint, decode.go:703-734): maxlen 8.  *big.Int (decodeBigInt, :271-287): any length
GSV_DI bool flat_uint_ok(const FlatView& b, const FItem& it, uint32_t maxlen) {
    return !it.list && it.n <= maxlen && !(it.n > 0 && b.at(it.off) == 0);
}

constexpr uint32_t TX_PATCH_NONE = 0xFFFFFFFFu;  // no segment is this long (items are <= 2^20 bytes)

// rlp.DecodeBytes(tx) over bytes [0, len), len in [1, 2^20]: whether it decodes, and where the six signed
// items lie: seg_lo .. seg_lo + seg_len (nonce's header to data's last byte), verbatim what both
// signers hash and what the signed transaction carries, because the decode rules leave one encoding per
// value, except a nil recipient sent as the empty list (0xc0), which rlp.Encode writes as 0x80:
// `patch` is that byte's offset in the segment, or TX_PATCH_NONE.  V, R and S only have to decode.
GSV_DI bool flat_tx_decode(const FlatView& b, uint32_t len, uint32_t& seg_lo, uint32_t& seg_len, uint32_t& patch) {
    FItem outer, f[9];
    uint32_t used = flat_rlp_item(b, 0, len, outer);
    bool ok = used && used == len && outer.list;
    uint32_t p = outer.off, rem = outer.n;
    for (int i = 0; i < 9 && ok; i++) {
        uint32_t u = flat_rlp_item(b, p, rem, f[i]);
        ok = u != 0;
        p += u;
        rem -= u;
    }
    ok = ok && rem == 0;
    ok = ok && flat_uint_ok(b, f[0], 8) && flat_uint_ok(b, f[2], 8) && flat_uint_ok(b, f[1], ~0u) &&
         flat_uint_ok(b, f[4], ~0u) && flat_uint_ok(b, f[6], ~0u) && flat_uint_ok(b, f[7], ~0u) &&
         flat_uint_ok(b, f[8], ~0u);
    // Recipient is rlp:"nil": size 0 of either kind is nil, else a 20-byte string
    ok = ok && (f[3].n == 0 || (!f[3].list && f[3].n == 20)) && !f[5].list;
    if (!ok) return false;
    seg_lo = f[0].start;
    seg_len = (f[5].off + f[5].n) - f[0].start;
    patch = f[3].list ? f[3].start - f[0].start : TX_PATCH_NONE;
    return true;
}

// The list header of an RLP payload of `body` bytes (< 2^24), in stream order: byte j of the header is
// byte j of the returned word; hlen <= 4
GSV_DI uint32_t list_header_le(uint32_t body, uint32_t& hlen) {
    if (body < 56) {
        hlen = 1;
        return 0xc0u + body;
    }
    uint32_t nb = body < 256 ? 1 : body < 65536 ? 2 : 3;
    hlen = 1 + nb;
    uint32_t be = __builtin_bswap32(body) >> (8u * (4u - nb));  // the nb length bytes, first byte lowest
    return (0xf7u + nb) | (be << 8);
}

// The stream [header][segment of the transaction, patched][tail].  Tail is a word array behind one zero
// word (tail byte j is byte 4 + j of the array), zero from the tail's end up to its last word + 1:
//   struct Tail { uint32_t word(uint32_t k) const; }   k <= (3 + tl) / 4 + 1
template <class Tail>
struct TxStream {
    FlatView b;
    uint32_t hdr, hlen;  // list_header_le
    uint32_t seg_lo, seg_len, patch;
    Tail tail;
    uint32_t tl;  // tail bytes
    GSV_DI uint32_t total() const { return hlen + seg_len + tl; }
    // stream bytes p .. p+3 as one little-endian word (any p), zero past the stream.  The segment's read
    // is unconditional (clamped into the item) and masked afterwards, so a block's loads issue together.
    GSV_DI uint32_t dword(uint32_t p) const {
        uint32_t out = p < 4u ? hdr >> (8u * p) : 0u;
        int32_t e = (int32_t)p - (int32_t)hlen;  // segment position of byte 0
        uint32_t q = e > 0 ? (uint32_t)e : 0u;
        uint32_t d = b.dword(seg_lo + q);
        uint32_t pd = patch - q;  // TX_PATCH_NONE - q stays >= 4
        if (pd < 4u) d ^= 0x40u << (8u * pd);  // 0xc0 -> 0x80
        // the first -e bytes are header (e >= -4, and -4 only for a four-byte header at p = 0)
        d = e < 0 ? (e > -4 ? d << (8u * (uint32_t)(-e)) : 0u) : d;
        int32_t vh = (int32_t)seg_len - e;  // bytes before the segment's end
        d = vh >= 4 ? d : vh > 0 ? d & ((1u << (8u * (uint32_t)vh)) - 1u) : 0u;
        out |= d;
        int32_t f = e - (int32_t)seg_len;  // tail position of byte 0
        int32_t fc = f < -4 ? -4 : f > (int32_t)tl ? (int32_t)tl : f;
        uint32_t fb = (uint32_t)(fc + 4);
        uint32_t t = __builtin_amdgcn_alignbyte(tail.word((fb >> 2) + 1u), tail.word(fb >> 2), fb & 3u);
        out |= (f > -4 && f < (int32_t)tl) ? t : 0u;
        return out;
    }
};

// Keccak-256 of the stream (crypto/sha3/sha3.go:98-157: rate 136, dsbyte 0x01), each rate block gathered
// as 34 words like notary.hip's keccak_stream.  Only a[0..3], the digest, are defined afterwards.
template <class Tail>
GSV_DI void keccak_tx_stream(uint64_t a[25], const TxStream<Tail>& s) {
#pragma unroll
    for (int k = 0; k < 25; k++) a[k] = 0;
    uint32_t len = s.total(), pos = 0;
    while (true) {
        uint32_t rem = len - pos;  // bytes left; the final block when rem < 136
        bool final = rem < 136;
#pragma unroll
        for (int w = 0; w < 17; w++) {
            uint64_t v = (uint64_t)s.dword(pos + 8u * w) | ((uint64_t)s.dword(pos + 8u * w + 4u) << 32);
            if (final && (rem >> 3) == (uint32_t)w) v ^= 0x01ull << (8u * (rem & 7u));
            if (final && w == 16) v ^= 0x8000000000000000ULL;
            a[w] ^= v;
        }
        if (final) break;
        keccakf(a);
        pos += 136;
    }
    keccakf_digest(a);
}

}  // namespace gsv

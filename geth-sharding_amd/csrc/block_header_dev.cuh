// types.Header on gfx950: the strict RLP decode of rlp.DecodeBytes into types.Header (core/types/block.go:70-86,
// rlp/decode.go), Keccak-256 over a header's bytes with a patched list head (Header.Hash / HashNoNonce,
// block.go:101-122), CalcDifficulty (consensus/ethash/consensus.go:297-459) in 256-bit limbs with a carry out,
// and the pieces of verifyHeader (consensus.go:223-285) that block_header.hip's kernels share.  Plain C++.
#pragma once
#include "block_header_host.h"
#include "ethash_dev.cuh"
#include "keccak_dev.cuh"

namespace gsv {
namespace bh {

// ---------------------------------------------------------------- 256-bit values
// A 32-byte big-endian row kept as the eight little-endian words of its bytes (as the hash rows are): limb j,
// least significant first, is bswap of word 7 - j.
struct U256 {
    uint32_t l[8];  // limbs, least significant first
};

GSV_DI U256 from_row(const uint32_t (&w)[8]) {
    U256 v;
#pragma unroll
    for (int j = 0; j < 8; j++) v.l[j] = __builtin_bswap32(w[7 - j]);
    return v;
}

GSV_DI void to_row(uint32_t (&w)[8], const U256& v) {
#pragma unroll
    for (int j = 0; j < 8; j++) w[7 - j] = __builtin_bswap32(v.l[j]);
}

GSV_DI U256 from_u64(uint64_t x) {
    U256 v;
    v.l[0] = (uint32_t)x;
    v.l[1] = (uint32_t)(x >> 32);
#pragma unroll
    for (int j = 2; j < 8; j++) v.l[j] = 0;
    return v;
}

GSV_DI uint64_t low64(const U256& v) { return (uint64_t)v.l[0] | (uint64_t)v.l[1] << 32; }

GSV_DI bool fits64(const U256& v) { return (v.l[2] | v.l[3] | v.l[4] | v.l[5] | v.l[6] | v.l[7]) == 0; }

// -1, 0, 1
GSV_DI int cmp(const U256& a, const U256& b) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) r = a.l[j] != b.l[j] ? (a.l[j] < b.l[j] ? -1 : 1) : r;
    return r;
}

// a + b, returns the carry out
GSV_DI bool add(U256& out, const U256& a, const U256& b) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (uint64_t)a.l[j] + b.l[j];
        out.l[j] = (uint32_t)c;
        c >>= 32;
    }
    return c != 0;
}

// a - b for a >= b
GSV_DI void sub(U256& out, const U256& a, const U256& b) {
    int64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        c += (int64_t)a.l[j] - (int64_t)b.l[j];
        out.l[j] = (uint32_t)c;
        c >>= 32;
    }
}

// a >> 11: the division by params.DifficultyBoundDivisor (2048)
GSV_DI U256 shr11(const U256& a) {
    U256 v;
#pragma unroll
    for (int j = 0; j < 8; j++) v.l[j] = (a.l[j] >> 11) | (j < 7 ? a.l[j + 1] << 21 : 0u);
    return v;
}

// a * b, returns whether the product is 2^256 or more (schoolbook columns, as ethash_dev.cuh pow_exceeds_target)
GSV_DI bool mul(U256& out, const U256& a, const U256& b) {
    uint64_t carry = 0;
    uint32_t high = 0;
#pragma unroll
    for (int col = 0; col < 15; col++) {
        uint64_t lo = carry & 0xFFFFFFFFull, hi = carry >> 32;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int j = col - i;
            if (j < 0 || j > 7) continue;
            const uint64_t p = (uint64_t)a.l[i] * b.l[j];
            lo += p & 0xFFFFFFFFull;
            hi += p >> 32;
        }
        hi += lo >> 32;
        if (col < 8) out.l[col] = (uint32_t)lo;
        else high |= (uint32_t)lo;
        carry = hi;
    }
    return (high | (uint32_t)carry | (uint32_t)(carry >> 32)) != 0;
}

// ceil(a / d) for a small d (9 or 10): long division from the top limb
GSV_DI U256 ceil_div_small(const U256& a, uint32_t d) {
    U256 q;
    uint64_t rem = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        const uint64_t cur = rem << 32 | a.l[j];
        q.l[j] = (uint32_t)(cur / d);
        rem = cur % d;
    }
    U256 r;
    add(r, q, from_u64(rem != 0));  // a / d < 2^253: no carry
    return r;
}

// ---------------------------------------------------------------- the decoded header
struct Header {
    uint32_t parent_hash[8], mix[8], difficulty[8], time[8];  // 32-byte rows as little-endian words
    uint64_t number, gas_limit, gas_used, nonce;
    uint32_t flags;    // block_header_host.h: decode status, uncle-hash flag, DAO-extra flag, len(Extra)
    uint32_t head;     // bytes of the list head (1 .. 5)
    uint32_t payload;  // bytes behind it
};

// types.EmptyUncleHash (core/types/block.go:36) = Keccak-256(rlp([])), as the little-endian words of its bytes
__device__ constexpr uint32_t EMPTY_UNCLE_HASH[8] = {0xe84dcc1du, 0x7a5dc7deu, 0x67b585abu, 0x1ad4ccb6u,
                                                     0x1b4512d3u, 0x13748a94u, 0xfd42a1f0u, 0x4793d440u};
// params.DAOForkBlockExtra (params/dao.go:28): "dao-hard-fork"
__device__ constexpr uint8_t DAO_EXTRA[13] = {0x64, 0x61, 0x6f, 0x2d, 0x68, 0x61, 0x72, 0x64, 0x2d, 0x66, 0x6f, 0x72, 0x6b};

// One string item of a list that ends at `end` (rlp/decode.go readKind :920-984 and Stream.Bytes' canonical-size
// rule): its content is p[off .. off + len), pos moves behind it.  false: no element left, a list where a string
// belongs, a length that reaches past the list, a long form for a short length, a leading zero in a length, or
// one byte below 0x80 in the long form ("81 05").
GSV_DI bool rlp_string(const uint8_t* __restrict__ p, uint32_t& pos, uint32_t end, uint32_t& off, uint32_t& len) {
    if (pos >= end) return false;
    const uint32_t b = p[pos];
    if (b < 0x80u) {
        off = pos;
        len = 1;
        pos += 1;
        return true;
    }
    if (b <= 0xB7u) {
        len = b - 0x80u;
        off = pos + 1;
        if (len > end - off) return false;
        if (len == 1 && p[off] < 0x80u) return false;
        pos = off + len;
        return true;
    }
    if (b > 0xBFu) return false;
    const uint32_t ll = b - 0xB7u;
    // more than four length bytes: 2^32 bytes or more, or leading zeros; either way no item of ours holds it
    if (ll > 4 || ll > end - (pos + 1)) return false;
    uint32_t size = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < ll; k++) size = size << 8 | p[pos + 1 + k];
    if (p[pos + 1] == 0 || size < 56) return false;
    off = pos + 1 + ll;
    if (size > end - off) return false;
    len = size;
    pos = off + size;
    return true;
}

// a byte array of exactly N bytes (decodeByteArray, rlp/decode.go:395-430)
template <int N>
GSV_DI bool rlp_fixed(const uint8_t* __restrict__ p, uint32_t& pos, uint32_t end, uint32_t& off) {
    uint32_t len;
    return rlp_string(p, pos, end, off, len) && len == (uint32_t)N;
}

GSV_DI void read_row32(uint32_t (&w)[8], const uint8_t* __restrict__ p) {
#pragma unroll
    for (int k = 0; k < 8; k++)
        w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 |
               (uint32_t)p[4 * k + 3] << 24;
}

// an integer of at most 32 bytes, right-aligned into a 32-byte big-endian row (compile-time word indices: no
// indexed register array)
GSV_DI void read_be_row(uint32_t (&w)[8], const uint8_t* __restrict__ p, uint32_t len) {
    const uint32_t pad = 32u - len;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t r = 4u * k + b;
            if (r >= pad) v |= (uint32_t)p[r - pad] << (8 * b);
        }
        w[k] = v;
    }
}

GSV_DI uint64_t read_be_u64(const uint8_t* __restrict__ p, uint32_t len) {
    uint64_t v = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < len; k++) v = v << 8 | p[k];
    return v;
}

// rlp.DecodeBytes(item, &types.Header{}) over p[0 .. len).  h.flags carries the verdict: GSV_ST_OK,
// GSV_ST_BAD_RLP for whatever the reference's decoder refuses, GSV_ST_HEADER_TOO_WIDE for a header that decodes
// but whose Difficulty or Time is wider than 32 bytes or whose Number is wider than 8.  No byte outside
// p[0 .. len) is read.
GSV_DI void decode_header(Header& h, const uint8_t* __restrict__ p, uint32_t len) {
    h.flags = GSV_ST_BAD_RLP;
    h.head = h.payload = 0;
    h.number = h.gas_limit = h.gas_used = h.nonce = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) h.parent_hash[k] = h.mix[k] = h.difficulty[k] = h.time[k] = 0;
    if (len == 0) return;
    const uint32_t b0 = p[0];
    if (b0 < 0xC0u) return;  // a string where the list belongs
    uint32_t head = 1, payload = b0 - 0xC0u;
    if (b0 > 0xF7u) {
        const uint32_t ll = b0 - 0xF7u;
        if (ll > 4 || 1 + ll > len) return;
        payload = 0;
#pragma unroll 1
        for (uint32_t k = 0; k < ll; k++) payload = payload << 8 | p[1 + k];
        if (p[1] == 0 || payload < 56) return;
        head = 1 + ll;
    }
    if (payload != len - head) return;  // truncated input, or bytes behind the list
    uint32_t pos = head, off, n;
    const uint32_t end = len;
    bool wide = false;
    uint32_t flags = 0;
    // ParentHash, UncleHash, Coinbase, Root, TxHash, ReceiptHash, Bloom
    if (!rlp_fixed<32>(p, pos, end, off)) return;
    read_row32(h.parent_hash, p + off);
    if (!rlp_fixed<32>(p, pos, end, off)) return;
    {
        uint32_t u[8], diff = 0;
        read_row32(u, p + off);
#pragma unroll
        for (int k = 0; k < 8; k++) diff |= u[k] ^ EMPTY_UNCLE_HASH[k];
        if (diff == 0) flags |= F_UNCLE_EMPTY;
    }
    if (!rlp_fixed<20>(p, pos, end, off)) return;
    if (!rlp_fixed<32>(p, pos, end, off)) return;
    if (!rlp_fixed<32>(p, pos, end, off)) return;
    if (!rlp_fixed<32>(p, pos, end, off)) return;
    if (!rlp_fixed<256>(p, pos, end, off)) return;
    // Difficulty, Number: decodeBigInt (rlp/decode.go:271-287), no leading zero byte
    if (!rlp_string(p, pos, end, off, n) || (n && p[off] == 0)) return;
    if (n > 32) wide = true;
    else read_be_row(h.difficulty, p + off, n);
    if (!rlp_string(p, pos, end, off, n) || (n && p[off] == 0)) return;
    if (n > 8) wide = true;
    else h.number = read_be_u64(p + off, n);
    // GasLimit, GasUsed: decodeUint (:239-247), at most 8 bytes
    if (!rlp_string(p, pos, end, off, n) || (n && p[off] == 0) || n > 8) return;
    h.gas_limit = read_be_u64(p + off, n);
    if (!rlp_string(p, pos, end, off, n) || (n && p[off] == 0) || n > 8) return;
    h.gas_used = read_be_u64(p + off, n);
    // Time
    if (!rlp_string(p, pos, end, off, n) || (n && p[off] == 0)) return;
    if (n > 32) wide = true;
    else read_be_row(h.time, p + off, n);
    // Extra: any string
    if (!rlp_string(p, pos, end, off, n)) return;
    flags |= (n < 0xFFFFu ? n : 0xFFFFu) << F_EXTRA_SHIFT;
    if (n == 13) {
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < 13; k++) diff |= (uint32_t)p[off + k] ^ DAO_EXTRA[k];
        if (diff == 0) flags |= F_DAO_EXTRA;
    }
    // MixDigest, Nonce
    if (!rlp_fixed<32>(p, pos, end, off)) return;
    read_row32(h.mix, p + off);
    if (!rlp_fixed<8>(p, pos, end, off)) return;
    h.nonce = read_be_u64(p + off, 8);  // Header.Nonce.Uint64(): the big-endian bytes as a number
    if (pos != end) return;             // a sixteenth element
    // MixDigest and Nonce took 42 bytes: a0 + 32 and 88 + 8
    h.head = head;
    h.payload = payload;
    h.flags = flags | (wide ? GSV_ST_HEADER_TOO_WIDE : GSV_ST_OK);
}

// ---------------------------------------------------------------- the two hashes
// Keccak-256 of the `len` bytes at `base` with the first `patch_len` (< 8) of them replaced by the low bytes of
// `patch`.  Reads the aligned dwords that hold a byte of base[0 .. len) and no other.
GSV_DI void keccak256_patched(uint32_t (&out)[8], const uint8_t* __restrict__ base, uint32_t len, uint64_t patch,
                              uint32_t patch_len) {
    const uint64_t keep = patch_len ? ~0ull << (8 * patch_len) : ~0ull;
    uint64_t a[25], w[17];
#pragma unroll
    for (int k = 0; k < 25; k++) a[k] = 0;
    uint32_t pos = 0;
    while (len - pos >= 136) {
        load_block(w, base + pos, 136);
        if (pos == 0) w[0] = (w[0] & keep) | patch;
#pragma unroll
        for (int k = 0; k < 17; k++) a[k] ^= w[k];
        keccakf(a);
        pos += 136;
    }
    const uint32_t rem = len - pos;
    load_block(w, base + pos, rem);
    if (pos == 0) w[0] = (w[0] & keep) | patch;
#pragma unroll
    for (int k = 0; k < 17; k++) {
        uint64_t x = w[k];
        if ((rem >> 3) == (uint32_t)k) x ^= 0x01ull << (8 * (rem & 7u));
        if (k == 16) x ^= 0x8000000000000000ULL;
        a[k] ^= x;
    }
    keccakf_digest(a);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        out[2 * k] = (uint32_t)a[k];
        out[2 * k + 1] = (uint32_t)(a[k] >> 32);
    }
}

// the list head of a payload of `payload` bytes (rlp/encode.go puthead) as the low bytes of a word; its length
GSV_DI uint32_t list_head(uint64_t& bytes, uint32_t payload) {
    if (payload < 56) {
        bytes = 0xC0u + payload;
        return 1;
    }
    const uint32_t ll = payload < 0x100u ? 1 : payload < 0x10000u ? 2 : payload < 0x1000000u ? 3 : 4;
    bytes = 0xF7u + ll;
#pragma unroll 1
    for (uint32_t k = 0; k < ll; k++) bytes |= (uint64_t)((payload >> (8 * (ll - 1 - k))) & 0xFFu) << (8 * (k + 1));
    return 1 + ll;
}

// ---------------------------------------------------------------- CalcDifficulty
// what the rules need of a parent
struct Parent {
    U256 difficulty, time;
    uint64_t number;
    bool uncle_empty;
};

// parent.Number + 1 >= fork, without wrapping
GSV_DI bool next_reaches(uint64_t parent_number, uint64_t fork) {
    return parent_number == ~0ull || parent_number + 1 >= fork;
}

// CalcDifficulty(config, time, parent) (consensus.go:297-459).  Returns true when the value is 2^256 or more
// (x is then unspecified): every step after an addition that carried only adds.
GSV_DI bool calc_difficulty(U256& x, const Config& cfg, uint64_t time, const Parent& p) {
    const bool byzantium = (cfg.flags & C_BYZANTIUM) && next_reaches(p.number, cfg.byzantium);
    const bool homestead = (cfg.flags & C_HOMESTEAD) && next_reaches(p.number, cfg.homestead);
    const U256 y = shr11(p.difficulty);  // parent_diff / 2048
    // time - parent.Time: negative when the parent's time is the larger one (verifyHeader never gets there, the
    // bare CalcDifficulty can)
    const bool negative = !fits64(p.time) || low64(p.time) > time;
    const uint64_t delta = time - low64(p.time);  // when !negative
    bool over = false;
    uint64_t period;
    if (!byzantium && !homestead) {
        // Frontier (:431-459): params.DurationLimit is 13
        if (negative || delta < 13) over = add(x, p.difficulty, y);
        else sub(x, p.difficulty, y);
        period = (p.number == ~0ull ? p.number : p.number + 1) / 100000u;  // 2^64 is no multiple of 100000
    } else {
        // Homestead (:382-426): max(1 - delta / 10, -99); Byzantium (:323-377): max((2 if uncles else 1) -
        // delta / 9, -99).  big.Int.Div is Euclidean: floor for a negative delta.
        const uint64_t base = byzantium ? (p.uncle_empty ? 1 : 2) : 1;
        U256 mag;
        bool minus = false;
        if (!negative) {
            const uint64_t q = byzantium ? delta / 9u : delta / 10u;
            if (q <= base) {
                mag = from_u64(base - q);
            } else {
                minus = true;
                mag = from_u64(q - base < 99 ? q - base : 99);
            }
        } else {
            U256 gap;
            sub(gap, p.time, from_u64(time));
            add(mag, ceil_div_small(gap, byzantium ? 9u : 10u), from_u64(base));
        }
        U256 prod;
        over = mul(prod, y, mag);
        if (minus) sub(x, p.difficulty, prod);  // 99 (d >> 11) < d
        else over |= add(x, p.difficulty, prod);
        if (byzantium) period = (p.number >= 2999999u ? p.number - 2999999u : 0) / 100000u;
        else period = (p.number == ~0ull ? p.number : p.number + 1) / 100000u;
    }
    if (over) return true;
    const U256 minimum = from_u64(131072);  // params.MinimumDifficulty
    if (cmp(x, minimum) < 0) x = minimum;
    if (period > 1) {
        // the bomb: 2^(period - 2)
        const uint64_t e = period - 2;
        if (e >= 256) return true;
        U256 bomb;
#pragma unroll
        for (int j = 0; j < 8; j++) bomb.l[j] = (e >> 5) == (uint64_t)j ? 1u << (e & 31u) : 0u;
        if (add(x, x, bomb)) return true;
    }
    return false;
}

}  // namespace bh
}  // namespace gsv

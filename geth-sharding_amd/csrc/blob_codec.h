// The blob codec's rules (sharding/utils/marshal.go:71-198), as plain text for host and device: the
// kernels of blob.hip and tests/native/blob_codec_host.cpp (g++, no HIP) run these same functions.
//
// Serialize (marshal.go:71-123).  A blob of L bytes becomes ceil(L / 31) chunks of 32 bytes:
//   non-terminal chunk c:  00 | data[31 c .. 31 c + 31)
//   terminal chunk:        tl | (skipEvm ? 0x80 : 0) | data[31 c .. 31 c + tl) | 31 - tl zero bytes
// with tl = L - 31 (chunks - 1) in [1, 31].  L = 0 gives no chunk at all (getNumChunks(0) = 0).
//
// Deserialize (marshal.go:144-198).  Only whole chunks count (a trailing partial chunk is ignored); a
// chunk whose indicator & 0x1F is tl != 0 ends a blob of 31 (chunks - 1) + tl bytes, bit 7 is its
// skipEvm flag, and no other indicator bit is read; chunks after the last terminal chunk are dropped.
//
// HOW NO LOAD LEAVES THE SOURCE.  A source buffer is described by a Src: the byte range [lo, hi) the
// caller owns, in offsets from a 4-byte aligned address at or below the buffer (so "aligned" is a
// property of the offset, whatever the buffer's own alignment).  Every source read goes through
// load_dword(): one aligned 4-byte load when the whole dword lies inside [lo, hi), else the bytes of it
// that do, one at a time.  Only the dword holding the range's first byte and the one holding its last
// can take that byte path; every other lane's loads are whole dwords.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GSV_BLOB_HD __host__ __device__ inline
#else
#define GSV_BLOB_HD inline
#endif

namespace gsv {
namespace blobc {

constexpr uint32_t CHUNK = 32;               // chunkSize
constexpr uint32_t CHUNK_DATA = 31;          // chunkDataSize
constexpr uint32_t GROUP = 16;               // bytes one lane writes: half a chunk, one dwordx4 store
constexpr uint64_t SIZE_LIMIT = 1ull << 20;  // collationSizelimit (sharding/collation.go:45)

// ---- plan arithmetic
GSV_BLOB_HD uint64_t num_chunks(uint64_t len) { return (len + CHUNK_DATA - 1) / CHUNK_DATA; }
GSV_BLOB_HD uint64_t serialized_size(uint64_t len) { return CHUNK * num_chunks(len); }
// SerializeTxToBlob's check (collation.go:169-171): a serialized size equal to the limit passes
GSV_BLOB_HD bool body_fits(uint64_t serialized_bytes) { return serialized_bytes <= SIZE_LIMIT; }

// per-blob entry of the serialize plan: where the blob lies and where its chunks go
struct BlobEnt {
    uint64_t off;    // blob bytes at blobs + off
    uint32_t len;    // L
    uint32_t first;  // first output chunk of the blob (counted over the whole batch)
};

// a source buffer: bytes [lo, hi) counted from the 4-aligned address `ab` (at least 4 below the
// buffer, so an offset one below a blob's start is still positive)
struct Src {
    const uint8_t* ab;
    uint64_t lo, hi, bias;
    GSV_BLOB_HD uint64_t at(uint64_t off) const { return off + bias; }  // buffer offset -> Src offset
};
GSV_BLOB_HD Src make_src(const uint8_t* base, uint64_t begin, uint64_t end) {
    const uint64_t bias = ((uintptr_t)base & 3) + 4;
    return Src{base - bias, begin + bias, end + bias, bias};
}

// little-endian dword at the 4-aligned offset p, reading no byte outside [lo, hi)
GSV_BLOB_HD uint32_t load_dword(const Src& s, uint64_t p) {
    if (p >= s.lo && p + 4 <= s.hi) {
        uint32_t v;
        memcpy(&v, __builtin_assume_aligned(s.ab + p, 4), 4);
        return v;
    }
    uint32_t v = 0;  // the range's first or last dword: byte path
    for (uint32_t k = 0; k < 4; k++)
        if (p + k >= s.lo && p + k < s.hi) v |= (uint32_t)s.ab[p + k] << (8 * k);
    return v;
}

// bytes [sh, sh + 4) of the 8-byte little-endian value hi:lo (sh in 0..4): the byte funnel shift
GSV_BLOB_HD uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
}

// ---- serialize: the four output words (little-endian) of half h (0, 1) of chunk c of the blob at
// buffer offset `off`, with length L and skipEvm flag f.  Chunk byte j is the indicator for j = 0, data
// byte 31 c + j - 1 for 1 <= j <= dl, and zero past that, whatever follows the blob in memory.
GSV_BLOB_HD void serialize_group(const Src& s, uint64_t off, uint32_t L, uint32_t f, uint32_t c, uint32_t h,
                                 uint32_t out[4]) {
    const uint32_t nch = (uint32_t)num_chunks(L);
    const bool term = c + 1 == nch;
    const uint32_t dl = term ? L - CHUNK_DATA * c : CHUNK_DATA;  // data bytes of this chunk, 1..31
    const uint32_t ind = term ? (dl | (f ? 0x80u : 0u)) : 0u;
    const uint64_t data = s.at(off) + (uint64_t)CHUNK_DATA * c;
    const uint64_t a = data + GROUP * h - 1;  // source of chunk byte 16 h
    const uint64_t p = a & ~(uint64_t)3;
    const uint32_t sh = (uint32_t)(a & 3);
    // a dword wholly past the chunk's data is not loaded; one that straddles its end is, and masked
    const uint64_t dend = data + dl;
    uint32_t d[5];
    for (uint32_t k = 0; k < 5; k++) d[k] = p + 4 * k < dend ? load_dword(s, p + 4 * k) : 0u;
    const uint32_t vb = 1 + dl;  // chunk bytes [0, vb) are indicator + data
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t j0 = GROUP * h + 4 * k;
        uint32_t w = funnel(d[k], d[k + 1], sh);
        const uint32_t nv = vb > j0 ? vb - j0 : 0;
        if (nv < 4) w &= (1u << (8 * nv)) - 1u;
        if (j0 == 0) w = (w & ~0xFFu) | ind;
        out[k] = w;
    }
}

// ---- deserialize: output word w (little-endian) of a body's data region, in which chunk c's 31 data
// bytes lie at 31 c (every indicator byte stripped; filler bytes copied as they stand).  The body has
// nch whole chunks from buffer offset `off`; bytes of the word at or past 31 nch are zero.
GSV_BLOB_HD uint32_t strip_word(const Src& s, uint64_t off, uint32_t nch, uint32_t w) {
    const uint32_t o = 4 * w, total = CHUNK_DATA * nch;
    if (o >= total) return 0;
    const uint32_t c = o / CHUNK_DATA, r = o - CHUNK_DATA * c;
    const uint64_t bend = s.at(off) + (uint64_t)CHUNK * nch;
    const uint64_t a = s.at(off) + o + c + 1;  // 32 c + 1 + r
    const uint64_t p = a & ~(uint64_t)3;
    const uint32_t sh = (uint32_t)(a & 3);
    // source bytes a .. a + 4 lie in two dwords (sh + 4 <= 7)
    const uint32_t d0 = load_dword(s, p);
    const uint32_t d1 = p + 4 < bend ? load_dword(s, p + 4) : 0u;
    uint32_t v = funnel(d0, d1, sh);
    const uint32_t nb = CHUNK_DATA - r;  // bytes left in chunk c from r on
    if (nb < 4) {
        // the word crosses into chunk c + 1, whose indicator lies between: those bytes are one further on
        const uint32_t m = (1u << (8 * nb)) - 1u;
        v = (v & m) | (funnel(d0, d1, sh + 1) & ~m);
    }
    const uint32_t nv = total - o;
    if (nv < 4) v &= (1u << (8 * nv)) - 1u;
    return v;
}

// ---- deserialize, the index half (what k_blob_index computes on the device), for the host round trip:
// blob t of a body of `len` bytes -> (first chunk, chunks, length, skipEvm); returns the blob count and
// writes the first `max` entries.
struct BlobSpan {
    uint32_t first_chunk, nchunks, len, skip_evm;
};
GSV_BLOB_HD uint32_t index_body(const uint8_t* body, uint64_t len, BlobSpan* out, uint32_t max) {
    const uint64_t nch = len / CHUNK;
    uint32_t n = 0, first = 0;
    for (uint64_t c = 0; c < nch; c++) {
        const uint8_t ind = body[CHUNK * c];
        const uint32_t tl = ind & 0x1Fu;
        if (!tl) continue;
        if (n < max) out[n] = BlobSpan{first, (uint32_t)c + 1 - first, CHUNK_DATA * ((uint32_t)c - first) + tl, (uint32_t)(ind >> 7)};
        n++;
        first = (uint32_t)c + 1;
    }
    return n;
}

}  // namespace blobc
}  // namespace gsv

// Kernels of the bloombits family (include/gsv.h, "bloombits"):
//   k_bb_generate    bloombits.Generator over whole sections: a bit-matrix transposition.  A workgroup takes a tile of
//                    512 blocks x 64 bloom bytes: every lane reads 32 blocks' dwords (16 lanes side by side cover 64
//                    contiguous bytes of one bloom), transposes sixteen 8 x 8 bit matrices in registers, and leaves 32
//                    dwords in a 32 KiB LDS tile laid out so that neither its stores nor the loads of the write-out
//                    meet a bank twice; the write-out stores 64 contiguous bytes of every one of the tile's 512 rows.
//   k_bb_compress    bitutil.CompressBytes: a wave per vector, the levels L, ceil(L / 8), .. , 1 in LDS, the length
//                    settled from the levels' popcounts before a byte is written.
//   k_bb_decompress  bitutil.DecompressBytes: a wave per vector, the levels from the innermost out, the first error
//                    of a level found as the minimum over the lanes.
//   k_bb_match       a wave per (query, section): the rule evaluation of bloombits_dev.cuh over words of 32 blocks.
//   k_bb_totals, k_bb_scan, k_bb_blocks   the matches as block numbers: each query's total, their scan, the numbers.
//   k_bb_filter      bloomFilter: a lane per (query, bloom), the same rule evaluation over a bloom's bytes.
#include "bloombits_dev.cuh"
#include "gsv_internal.h"

namespace gsv {

using namespace bb;

namespace {

constexpr uint32_t TILE_BLOCKS = 512, TILE_COLS = 64;  // one workgroup of k_bb_generate
constexpr uint32_t TILE_ROWS = TILE_COLS * 8;          // bit rows of a tile: 512 rows x 16 dwords of LDS
constexpr uint32_t COL_TILES = BLOOM_BYTES / TILE_COLS;

// LDS place of dword column jq (32 blocks) of tile row lr: rows in pairs swap places for odd jq and the columns are
// XORed with the row's dword column group lr >> 5, so the 32 lanes of a store (16 column groups x 2 jq) and of a
// load of the write-out (2 rows x 16 jq) each meet 32 different banks.
GSV_DI uint32_t tile_at(uint32_t lr, uint32_t jq) { return ((lr ^ (jq & 1u)) << 4) | (jq ^ (lr >> 5)); }

__global__ __launch_bounds__(256) void k_bb_generate(const uint8_t* __restrict__ blooms, uint32_t S, uint32_t tiles_j,
                                                     uint8_t* __restrict__ bits, int in_fast, int out_fast) {
    __shared__ uint32_t tile[TILE_ROWS * 16];
    const uint32_t ct = blockIdx.x % COL_TILES, jt = (blockIdx.x / COL_TILES) % tiles_j;
    const uint64_t sec = blockIdx.x / COL_TILES / tiles_j;
    const uint32_t cd = threadIdx.x & 15u, jq = threadIdx.x >> 4;
    const uint32_t rb = S / 8, j0 = jt * TILE_BLOCKS + jq * 32u, c0 = ct * TILE_COLS + cd * 4u;
    uint32_t v[32];
    const uint8_t* src = blooms + (sec * S + j0) * BLOOM_BYTES + c0;
#pragma unroll
    for (uint32_t k = 0; k < 32; k++) {
        v[k] = 0;
        if (j0 + k < S) {
            const uint8_t* p = src + (size_t)k * BLOOM_BYTES;
            if (in_fast) v[k] = *(const uint32_t*)p;
            else v[k] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        }
    }
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (uint32_t g = 0; g < 4; g++) {
            // block j0 + 8 g + k in byte 7 - k: row 7 - k of the matrix, so that column p (bit p of the bloom byte)
            // comes out as byte p with block k under mask 1 << (7 - k) (generator.go:61-62)
            uint64_t x = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) x |= (uint64_t)((v[8 * g + k] >> (8 * b)) & 0xFFu) << (8 * (7 - k));
            x = transpose8(x);
#pragma unroll
            for (uint32_t p = 0; p < 8; p++) w[p] |= (uint32_t)((x >> (8 * p)) & 0xFFu) << (8 * g);
        }
#pragma unroll
        for (uint32_t p = 0; p < 8; p++) tile[tile_at((cd * 4u + b) * 8u + p, jq)] = w[p];
    }
    __syncthreads();
    // tile row lr: byte column ct * 64 + lr / 8 of the bloom, bit lr % 8 of it: bloom bit (255 - column) * 8 + lr % 8
    const uint32_t oq = threadIdx.x & 15u, byte0 = jt * (TILE_BLOCKS / 8) + oq * 4u;
#pragma unroll 4
    for (uint32_t it = 0; it < TILE_ROWS / 16; it++) {
        const uint32_t lr = it * 16u + (threadIdx.x >> 4);
        const uint32_t bit = (BLOOM_BYTES - 1u - (ct * TILE_COLS + lr / 8u)) * 8u + (lr & 7u);
        const uint32_t val = tile[tile_at(lr, oq)];
        uint8_t* row = bits + (sec * BLOOM_BITS + bit) * rb;
        if (out_fast) {
            if (byte0 < rb) *(uint32_t*)(row + byte0) = val;
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if (byte0 + b < rb) row[byte0 + b] = (uint8_t)(val >> (8 * b));
        }
    }
}

// ---- the codec.  LDS of one wave: the levels back to back, each padded to a multiple of 8 bytes with zeros.
constexpr uint32_t MAX_LEVELS = 5;                                  // 4096, 512, 64, 8, 1
constexpr uint32_t LEVEL_WORDS = (4096 + 512 + 64 + 8 + 8) / 4;

struct Levels {
    uint32_t n, len[MAX_LEVELS], at[MAX_LEVELS];  // at: byte offset in LDS
};
GSV_DI Levels make_levels(uint32_t L) {
    Levels lv;
    lv.n = 0;
    uint32_t at = 0;
#pragma unroll
    for (uint32_t k = 0; k < MAX_LEVELS; k++) {
        lv.len[k] = 0;
        lv.at[k] = 0;
    }
#pragma unroll
    for (uint32_t k = 0; k < MAX_LEVELS; k++) {
        lv.len[k] = L;
        lv.at[k] = at;
        lv.n = k + 1;
        at += (L + 7u) & ~7u;
        if (L <= 1) break;
        L = (L + 7u) / 8u;
    }
    return lv;
}

__global__ __launch_bounds__(64) void k_bb_compress(const uint8_t* __restrict__ in, uint32_t L,
                                                    uint8_t* __restrict__ slots, uint32_t* __restrict__ out_len) {
    __shared__ uint32_t ldsw[LEVEL_WORDS];
    uint8_t* lds = (uint8_t*)ldsw;
    const uint32_t lane = threadIdx.x;
    const size_t i = blockIdx.x;
    const Levels lv = make_levels(L);
    for (uint32_t k = lane; k < LEVEL_WORDS; k += 64) ldsw[k] = 0;
    __syncthreads();
    const uint8_t* vec = in + i * L;
    const bool fast = (((uintptr_t)vec | L) & 3u) == 0;
    for (uint32_t w = lane; w < (L + 3u) / 4u; w += 64) ldsw[w] = row_word(vec, w, L, fast);
    __syncthreads();
    // the bitset of every level (compress.go:84-92) and its count of non-zero bytes
    uint32_t nz[MAX_LEVELS] = {0, 0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t k = 0; k + 1 < lv.n; k++) {
        const uint8_t* cur = lds + lv.at[k];
        uint8_t* nxt = lds + lv.at[k + 1];
        uint32_t cnt = 0;
        for (uint32_t b = lane; b < lv.len[k + 1]; b += 64) {
            uint32_t m = 0;
#pragma unroll
            for (uint32_t t = 0; t < 8; t++) m |= (cur[8 * b + t] != 0 ? 1u : 0u) << (7 - t);
            nxt[b] = (uint8_t)m;
            cnt += __popc(m);
        }
        nz[k] = wave_sum(cnt);
        __syncthreads();
    }
    nz[lv.n - 1] = lds[lv.at[lv.n - 1]] != 0 ? 1u : 0u;  // the level of one byte (compress.go:77-82)
    uint32_t total = 0;
#pragma unroll
    for (uint32_t k = 0; k < MAX_LEVELS; k++) total += nz[k];
    uint8_t* slot = slots + i * L;
    if (nz[0] == 0) {  // compress.go:93-95 (and :78-80)
        if (lane == 0) out_len[i] = 0;
        return;
    }
    if (total >= L) {  // compress.go:61-66: the encoding is not shorter
        const bool sfast = (((uintptr_t)slot | L) & 3u) == 0;
        for (uint32_t w = lane; w < (L + 3u) / 4u; w += 64) row_word_store(slot, w, L, sfast, ldsw[w]);
        if (lane == 0) out_len[i] = L;
        return;
    }
    // compress.go:96: the innermost level first.  total < L: every store below lies inside the slot
    if (lane == 0) {
        out_len[i] = total;
        slot[0] = lds[lv.at[lv.n - 1]];
    }
    uint32_t at = 1;
#pragma unroll 1
    for (int k = (int)lv.n - 2; k >= 0; k--) {
        const uint8_t* cur = lds + lv.at[k];
        const uint8_t* set = lds + lv.at[k + 1];
        uint32_t base = at;
        for (uint32_t b0 = 0; b0 < lv.len[k + 1]; b0 += 64) {
            const uint32_t b = b0 + lane;
            const uint32_t m = b < lv.len[k + 1] ? set[b] : 0u;
            const uint32_t inc = wave_scan(__popc(m));
            uint32_t pos = base + inc - __popc(m);
#pragma unroll
            for (uint32_t t = 0; t < 8; t++)
                if (m & (0x80u >> t)) slot[pos++] = cur[8 * b + t];
            base += __shfl(inc, 63, 64);
        }
        at += nz[k];
    }
}

__global__ __launch_bounds__(64) void k_bb_decompress(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                      uint32_t L, uint8_t* __restrict__ out,
                                                      uint8_t* __restrict__ status) {
    __shared__ uint32_t ldsw[LEVEL_WORDS];
    uint8_t* lds = (uint8_t*)ldsw;
    const uint32_t lane = threadIdx.x;
    const size_t i = blockIdx.x;
    const Levels lv = make_levels(L);
    for (uint32_t k = lane; k < LEVEL_WORDS; k += 64) ldsw[k] = 0;
    __syncthreads();
    uint8_t* row = out + i * L;
    const bool rfast = (((uintptr_t)row | L) & 3u) == 0;
    const uint64_t o0 = off[i], o1 = off[i + 1];
    const uint8_t* d = data + o0;
    uint32_t st = GSV_ST_OK;
    if (o1 < o0) st = GSV_ST_BITSET_MISSING_DATA;         // ours: a table that steps backwards
    else if (o1 - o0 > L) st = GSV_ST_BITSET_EXCEEDED_TARGET;  // compress.go:103-105
    const uint32_t len = st ? 0u : (uint32_t)(o1 - o0);
    if (!st && len == L) {  // compress.go:106-110
        for (uint32_t k = lane; k < L; k += 64) lds[k] = d[k];
    } else if (!st && len != 0) {  // len == 0: zeros (compress.go:137-139)
        // the level of one byte (:140-146), then every level from its bitset (:148-168)
        const uint8_t top = d[0];
        if (lane == 0) lds[lv.at[lv.n - 1]] = top;
        uint32_t ptr = top != 0 ? 1u : 0u;
        __syncthreads();
#pragma unroll 1
        for (int k = (int)lv.n - 2; k >= 0 && !st; k--) {
            uint8_t* cur = lds + lv.at[k];
            const uint8_t* set = lds + lv.at[k + 1];
            const uint32_t target = lv.len[k];
            uint32_t bad = 0xFFFFFFFFu;  // 4 x the first failing bit's index + which check failed
            for (uint32_t b0 = 0; b0 < lv.len[k + 1]; b0 += 64) {
                const uint32_t b = b0 + lane;
                const uint32_t m = b < lv.len[k + 1] ? set[b] : 0u;
                const uint32_t inc = wave_scan(__popc(m));
                uint32_t p = ptr + inc - __popc(m);
#pragma unroll
                for (uint32_t t = 0; t < 8; t++)
                    if (m & (0x80u >> t)) {
                        const uint32_t idx = 8 * b + t;
                        if (p >= len) bad = min(bad, 4 * idx);                 // :155-157
                        else if (idx >= target) bad = min(bad, 4 * idx + 1);   // :158-160
                        else {
                            const uint8_t x = d[p];
                            if (x == 0) bad = min(bad, 4 * idx + 2);           // :162-164
                            else cur[idx] = x;
                        }
                        p++;
                    }
                ptr += __shfl(inc, 63, 64);
            }
            bad = wave_min(bad);
            if (bad != 0xFFFFFFFFu)
                st = (bad & 3u) == 0 ? GSV_ST_BITSET_MISSING_DATA
                                     : (bad & 3u) == 1 ? GSV_ST_BITSET_EXCEEDED_TARGET : GSV_ST_BITSET_ZERO_CONTENT;
            __syncthreads();
        }
        if (!st && ptr != len) st = GSV_ST_BITSET_UNREFERENCED_DATA;  // :120-122
    }
    __syncthreads();
    for (uint32_t w = lane; w < (L + 3u) / 4u; w += 64) row_word_store(row, w, L, rfast, st ? 0u : ldsw[w]);
    if (lane == 0) status[i] = (uint8_t)st;
}

// ---- the matcher
__global__ __launch_bounds__(256) void k_bb_match(const uint8_t* __restrict__ bits, uint32_t S, uint64_t first_section,
                                                  uint32_t n_sections, const uint16_t* __restrict__ clauses,
                                                  uint32_t n_clauses, const uint32_t* __restrict__ rule_off,
                                                  uint32_t n_rules, const uint32_t* __restrict__ query_off,
                                                  uint32_t n_queries, const uint64_t* __restrict__ begin,
                                                  const uint64_t* __restrict__ end, uint8_t* __restrict__ match,
                                                  uint32_t* __restrict__ count, int fast, int mfast) {
    const uint32_t pair = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (pair >= n_queries * n_sections) return;
    const uint32_t q = pair / n_sections, s = pair % n_sections, rb = S / 8;
    const uint32_t r0 = query_off[q], r1 = query_off[q + 1];
    const uint64_t lo = begin[q], hi = end[q], block0 = (first_section + s) * S;
    const uint8_t* table = bits + (uint64_t)s * BLOOM_BITS * rb;
    uint8_t* mrow = match + (uint64_t)pair * rb;
    uint32_t cnt = 0;
    for (uint32_t w = lane; w < (rb + 3u) / 4u; w += 64) {
        uint32_t v = eval_query(clauses, n_clauses, rule_off, n_rules, r0, r1,
                                [&](uint32_t bit) { return row_word(table + (uint64_t)bit * rb, w, rb, fast); });
        uint32_t keep = 0;  // matcher.go:182-192, and the bytes behind a row that is no whole number of words
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (4 * w + b < rb) keep |= range_mask8(block0 + 8ull * (4 * w + b), lo, hi) << (8 * b);
        v &= keep;
        row_word_store(mrow, w, rb, mfast, v);
        cnt += __popc(v);
    }
    cnt = wave_sum(cnt);
    if (lane == 0) count[pair] = cnt;
}

__global__ __launch_bounds__(256) void k_bb_totals(const uint32_t* __restrict__ count, uint32_t n_sections,
                                                   uint32_t n_queries, uint64_t* __restrict__ block_off) {
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= n_queries) return;
    uint64_t total = 0;  // up to 2^20 sections of 2^15 blocks
    for (uint32_t s = lane; s < n_sections; s += 64) total += count[(uint64_t)q * n_sections + s];
    total = wave_sum64(total);
    if (lane == 0) {
        block_off[q + 1] = total;
        if (q == 0) block_off[0] = 0;
    }
}

// one workgroup: block_off[1 .. n] summed in place, 1024 at a time behind a running carry
__global__ __launch_bounds__(1024) void k_bb_scan(uint64_t* __restrict__ block_off, uint32_t n_queries) {
    __shared__ uint64_t sh[1024];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t q0 = 0; q0 < n_queries; q0 += 1024) {
        const uint32_t q = q0 + threadIdx.x;
        uint64_t v = q < n_queries ? block_off[q + 1] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint64_t o = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            v += o;
            sh[threadIdx.x] = v;
            __syncthreads();
        }
        if (q < n_queries) block_off[q + 1] = carry + v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bb_blocks(const uint8_t* __restrict__ match, const uint32_t* __restrict__ count,
                                                   uint32_t S, uint64_t first_section, uint32_t n_sections,
                                                   uint32_t n_queries, const uint64_t* __restrict__ block_off,
                                                   uint64_t* __restrict__ blocks, uint64_t capacity, int mfast) {
    const uint32_t pair = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (pair >= n_queries * n_sections) return;
    const uint32_t q = pair / n_sections, s = pair % n_sections, rb = S / 8;
    if (count[pair] == 0) return;
    // where this section's numbers start: behind those of the query's sections before it
    uint64_t base = 0;
    for (uint32_t k = lane; k < s; k += 64) base += count[(uint64_t)q * n_sections + k];
    base = wave_sum64(base) + block_off[q];
    const uint8_t* mrow = match + (uint64_t)pair * rb;
    const uint64_t block0 = (first_section + s) * S;
    for (uint32_t w0 = 0; w0 < (rb + 3u) / 4u; w0 += 64) {
        const uint32_t w = w0 + lane;
        const uint32_t v = w < (rb + 3u) / 4u ? row_word(mrow, w, rb, mfast) : 0u;
        const uint32_t inc = wave_scan(__popc(v));
        uint64_t pos = base + inc - __popc(v);
        if (v) {
#pragma unroll 1
            for (uint32_t b = 0; b < 4; b++) {
                const uint32_t x = (v >> (8 * b)) & 0xFFu;
                for (uint32_t t = 0; t < 8 && x; t++)
                    if (x & (0x80u >> t)) {  // matcher.go:204
                        if (pos < capacity) blocks[pos] = block0 + 8ull * (4 * w + b) + t;
                        pos++;
                    }
            }
        }
        base += __shfl(inc, 63, 64);
    }
}

__global__ __launch_bounds__(256) void k_bb_filter(const uint8_t* __restrict__ blooms, uint32_t n_blooms,
                                                   const uint16_t* __restrict__ clauses, uint32_t n_clauses,
                                                   const uint32_t* __restrict__ rule_off, uint32_t n_rules,
                                                   const uint32_t* __restrict__ query_off, uint32_t n_queries,
                                                   uint8_t* __restrict__ out) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)n_queries * n_blooms) return;
    const uint32_t q = (uint32_t)(idx / n_blooms);
    const uint8_t* bloom = blooms + (idx % n_blooms) * BLOOM_BYTES;
    const uint32_t v = eval_query(clauses, n_clauses, rule_off, n_rules, query_off[q], query_off[q + 1],
                                  [&](uint32_t bit) {  // BloomLookup: bloom9.go:131-136 in generator.go:64-70's numbering
                                      return (bloom[BLOOM_BYTES - 1u - bit / 8u] >> (bit & 7u)) & 1u ? 0xFFFFFFFFu : 0u;
                                  });
    out[idx] = v ? 1 : 0;
}

}  // namespace

hipError_t launch_bloombits_generate(const uint8_t* d_blooms, uint32_t n_sections, uint32_t S, uint8_t* d_bits,
                                     hipStream_t st) {
    if (n_sections == 0) return hipSuccess;
    const uint32_t tiles_j = (S + TILE_BLOCKS - 1) / TILE_BLOCKS, rb = S / 8;
    const int in_fast = ((uintptr_t)d_blooms & 3u) == 0;
    const int out_fast = (((uintptr_t)d_bits | rb) & 3u) == 0;
    hipLaunchKernelGGL(k_bb_generate, dim3(n_sections * tiles_j * COL_TILES), dim3(256), 0, st, d_blooms, S, tiles_j,
                       d_bits, in_fast, out_fast);
    return hipGetLastError();
}

hipError_t launch_bitset_compress(const uint8_t* d_in, uint32_t n, uint32_t L, uint8_t* d_slots, uint32_t* d_len,
                                  hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bb_compress, dim3(n), dim3(64), 0, st, d_in, L, d_slots, d_len);
    return hipGetLastError();
}

hipError_t launch_bitset_decompress(const uint8_t* d_data, const uint64_t* d_off, uint32_t n, uint32_t L, uint8_t* d_out,
                                    uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bb_decompress, dim3(n), dim3(64), 0, st, d_data, d_off, L, d_out, d_status);
    return hipGetLastError();
}

hipError_t launch_bloombits_match(const uint8_t* d_bits, uint32_t S, uint64_t first_section, uint32_t n_sections,
                                  const uint16_t* d_clauses, uint32_t n_clauses, const uint32_t* d_rule_off,
                                  uint32_t n_rules, const uint32_t* d_query_off, uint32_t n_queries,
                                  const uint64_t* d_begin, const uint64_t* d_end, uint8_t* d_match, uint32_t* d_count,
                                  hipStream_t st) {
    const uint32_t pairs = n_queries * n_sections, rb = S / 8;
    if (pairs == 0) return hipSuccess;
    const int fast = (((uintptr_t)d_bits | rb) & 3u) == 0, mfast = (((uintptr_t)d_match | rb) & 3u) == 0;
    hipLaunchKernelGGL(k_bb_match, dim3((pairs + 3) / 4), dim3(256), 0, st, d_bits, S, first_section, n_sections,
                       d_clauses, n_clauses, d_rule_off, n_rules, d_query_off, n_queries, d_begin, d_end, d_match,
                       d_count, fast, mfast);
    return hipGetLastError();
}

hipError_t launch_bloombits_totals(const uint32_t* d_count, uint32_t n_sections, uint32_t n_queries,
                                   uint64_t* d_block_off, hipStream_t st) {
    hipLaunchKernelGGL(k_bb_totals, dim3((n_queries + 3) / 4), dim3(256), 0, st, d_count, n_sections, n_queries,
                       d_block_off);
    return hipGetLastError();
}

hipError_t launch_bloombits_scan(uint64_t* d_block_off, uint32_t n_queries, hipStream_t st) {
    hipLaunchKernelGGL(k_bb_scan, dim3(1), dim3(1024), 0, st, d_block_off, n_queries);
    return hipGetLastError();
}

hipError_t launch_bloombits_blocks(const uint8_t* d_match, const uint32_t* d_count, uint32_t S, uint64_t first_section,
                                   uint32_t n_sections, uint32_t n_queries, const uint64_t* d_block_off,
                                   uint64_t* d_blocks, uint64_t capacity, hipStream_t st) {
    const uint32_t pairs = n_queries * n_sections, rb = S / 8;
    if (pairs == 0) return hipSuccess;
    const int mfast = (((uintptr_t)d_match | rb) & 3u) == 0;
    hipLaunchKernelGGL(k_bb_blocks, dim3((pairs + 3) / 4), dim3(256), 0, st, d_match, d_count, S, first_section,
                       n_sections, n_queries, d_block_off, d_blocks, capacity, mfast);
    return hipGetLastError();
}

hipError_t launch_bloom_filter(const uint8_t* d_blooms, uint32_t n_blooms, const uint16_t* d_clauses, uint32_t n_clauses,
                               const uint32_t* d_rule_off, uint32_t n_rules, const uint32_t* d_query_off,
                               uint32_t n_queries, uint8_t* d_out, hipStream_t st) {
    const uint64_t total = (uint64_t)n_queries * n_blooms;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bb_filter, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, d_blooms, n_blooms,
                       d_clauses, n_clauses, d_rule_off, n_rules, d_query_off, n_queries, d_out);
    return hipGetLastError();
}

}  // namespace gsv

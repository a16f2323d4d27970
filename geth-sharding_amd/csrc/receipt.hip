// Batched receipt validation: the receipt half of BlockValidator.ValidateState (core/block_validator.go:80-95)
// over RLP-encoded consensus receipts, and bloom9 over arbitrary byte strings.
//
//   k_receipt_scan    one receipt per lane: rlp.DecodeBytes into types.Receipt (receipt_dev.cuh), its status,
//                     CumulativeGasUsed, the list it belongs to, and one descriptor per log address and topic in a
//                     zero-filled table of one slot per 21 bytes of RLP, written as the decode walks.  A receipt
//                     that fails is walked once more to take its descriptors back: it contributes none.
//   k_receipt_bloom   one BLOOM ITEM per lane, never one receipt: a workgroup takes 2,048 slots, compacts the
//                     items it finds into LDS and runs them 256 at a time, so a receipt of hundreds of logs is
//                     spread over lanes like any other.  One digest permutation per item, three bits ORed into
//                     the list's row (through an LDS row for the list most of the workgroup's items belong to) and,
//                     where asked for, the receipt's row.
//   k_receipt_lists   one list per wave: the first failing receipt's status, gas used, and zeros over the bloom
//                     row of a list that holds a failed receipt
//   k_receipt_check   one list per lane: gas used, bloom and receipt root against the header's, in
//                     ValidateState's order
//   k_bloom9          one message per lane: calcBloomIndexes (bloom9.go:115-127), any length
//
// The receipt root between k_receipt_lists and k_receipt_check is DeriveSha over the same bytes (the decoder
// accepts canonical encodings only, so what decodes re-encodes to itself): chunk_root.hip's kernels.
#include "gsv_internal.h"
#include "receipt_dev.cuh"

namespace gsv {

using namespace rc;

namespace {

constexpr uint32_t BLOOM_WG_SLOTS = 2048;  // slots of one k_receipt_bloom workgroup: 16 KiB of LDS
constexpr uint32_t NO_LIST = 0xFFFFFFFFu;

// the list that holds receipt i: the last one whose first receipt is at or before i (empty lists share a
// start with the list behind them).  list_off has n_lists + 1 ascending entries.
GSV_DI uint32_t list_of(const uint64_t* __restrict__ list_off, uint32_t n_lists, uint32_t i) {
    if (i < list_off[0] || i >= list_off[n_lists]) return NO_LIST;
    uint32_t lo = 0, hi = n_lists;  // list_off[lo] <= i < list_off[hi]
#pragma unroll 1
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace

// Receipt i is vals[voff[i] .. voff[i + 1]).  OURS, not the reference's: a receipt that starts before
// voff[0], ends before it starts, is 2^32 bytes or longer, or ends more than vals_bytes behind voff[0] is
// GSV_ST_BAD_RLP unread, so no descriptor lands outside the table of vals_bytes / 21 + 1 slots.
__global__ __launch_bounds__(256) void k_receipt_scan(const uint8_t* __restrict__ vals,
                                                      const uint64_t* __restrict__ voff, uint32_t n,
                                                      const uint64_t* __restrict__ list_off, uint32_t n_lists,
                                                      uint64_t vals_bytes, uint64_t* __restrict__ desc,
                                                      uint64_t* __restrict__ gas, uint32_t* __restrict__ list_idx,
                                                      uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t v0 = voff[0], a = voff[i], b = voff[i + 1];
    uint64_t g = 0;
    uint32_t st = GSV_ST_BAD_RLP;
    if (a >= v0 && b >= a && b - a <= 0xFFFFFFFFull && b - v0 <= vals_bytes) {
        const uint8_t* p = vals + a;
        const uint32_t len = (uint32_t)(b - a);
        st = decode_receipt<false>(p, len, g, desc, a - v0, i);
        if (st != GSV_ST_OK) {
            uint64_t unused;
            decode_receipt<true>(p, len, unused, desc, a - v0, i);
        }
    }
    gas[i] = g;
    list_idx[i] = list_of(list_off, n_lists, i);
    status[i] = (uint8_t)st;
}

// slots: vals_bytes / 21 + 1.  list_bloom / receipt_bloom: rows of 256 bytes at any alignment, zero-filled
// before the launch (receipt_bloom null: not wanted).
__global__ __launch_bounds__(256) void k_receipt_bloom(const uint8_t* __restrict__ vals,
                                                       const uint64_t* __restrict__ voff,
                                                       const uint64_t* __restrict__ desc, uint64_t slots,
                                                       const uint32_t* __restrict__ list_idx,
                                                       uint8_t* __restrict__ list_bloom,
                                                       uint8_t* __restrict__ receipt_bloom) {
    __shared__ uint32_t s_at[BLOOM_WG_SLOTS], s_receipt[BLOOM_WG_SLOTS];
    __shared__ uint32_t s_row[64], s_count, s_list;
    const uint32_t t = threadIdx.x;
    const uint64_t slot0 = (uint64_t)blockIdx.x * BLOOM_WG_SLOTS;
    if (t == 0) s_count = 0, s_list = NO_LIST;
    if (t < 64) s_row[t] = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < BLOOM_WG_SLOTS / 256; j++) {
        const uint32_t local = j * 256 + t;
        const uint64_t d = slot0 + local < slots ? desc[slot0 + local] : 0;
        if (d & D_VALID) {
            const uint32_t k = atomicAdd(&s_count, 1u);
            s_at[k] = (local * SLOT_BYTES + ((uint32_t)(d >> D_DELTA_SHIFT) & 31u)) | (d & D_TOPIC ? 1u << 31 : 0);
            s_receipt[k] = (uint32_t)d;
        }
    }
    __syncthreads();
    const uint32_t count = s_count;
    if (count == 0) return;  // uniform
    // the workgroup's own row: the list of one of its items (a workgroup's slots are 43,008 consecutive bytes
    // of RLP, so most of its items share a list)
    if (t == 0) s_list = list_idx[s_receipt[0]];
    __syncthreads();
    const uint32_t own = s_list;
    const uint8_t* base = vals + voff[0] + slot0 * SLOT_BYTES;
#pragma unroll 1
    for (uint32_t k = t; k < count; k += 256) {
        const uint32_t at = s_at[k] & 0x7FFFFFFFu, receipt = s_receipt[k];
        const uint64_t h = item_digest(base + at + 1, (s_at[k] >> 31) != 0);
        const uint32_t list = list_idx[receipt];
#pragma unroll
        for (int x = 0; x < 3; x++) {
            const uint32_t b = bloom_index(h, x);
            // bit b: byte 255 - b / 8 of the row, here as bit 8 (byte % 4) + b % 8 of word byte / 4
            const uint32_t byte = 255u - (b >> 3);
            if (list == own) atomicOr(&s_row[byte >> 2], (1u << (b & 7u)) << (8u * (byte & 3u)));
            else if (list != NO_LIST) bloom_or_bit(list_bloom + (size_t)list * 256, b);
            if (receipt_bloom) bloom_or_bit(receipt_bloom + (size_t)receipt * 256, b);
        }
    }
    __syncthreads();
    if (own == NO_LIST) return;
    // the row's bytes that hold a bit, one byte per thread
    const uint32_t mine = (s_row[t >> 2] >> (8u * (t & 3u))) & 0xFFu;
    if (mine) {
        const uintptr_t at = (uintptr_t)(list_bloom + (size_t)own * 256 + t);
        atomicOr((uint32_t*)(at & ~(uintptr_t)3), mine << (8u * (uint32_t)(at & 3u)));
    }
}

// One wave per list (four lists per workgroup).  list_status[L]: the status of the first receipt of list L
// that is not GSV_ST_OK, else GSV_ST_OK; gas_used[L]: the last receipt's CumulativeGasUsed, 0 for an empty
// list and for one with a failed receipt, whose bloom row is overwritten with zeros too.
__global__ __launch_bounds__(256) void k_receipt_lists(const uint64_t* __restrict__ list_off, uint32_t n_lists,
                                                       uint32_t n, const uint8_t* __restrict__ receipt_status,
                                                       const uint64_t* __restrict__ gas,
                                                       uint8_t* __restrict__ list_bloom,
                                                       uint64_t* __restrict__ gas_used,
                                                       uint8_t* __restrict__ list_status) {
    const uint32_t L = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63u;
    if (L >= n_lists) return;
    uint64_t a = list_off[L], b = list_off[L + 1];
    b = b < n ? b : n;
    a = a < b ? a : b;
    uint32_t first = 0xFFFFFFFFu;
#pragma unroll 1
    for (uint64_t k = a + lane; k < b && first == 0xFFFFFFFFu; k += 64)
        if (receipt_status[k] != GSV_ST_OK) first = (uint32_t)k;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)first, w, 64);
        first = other < first ? other : first;
    }
    const bool failed = first != 0xFFFFFFFFu;
    if (lane == 0) {
        list_status[L] = failed ? receipt_status[first] : (uint8_t)GSV_ST_OK;
        gas_used[L] = !failed && b > a ? gas[b - 1] : 0;
    }
    if (failed) {
        uint8_t* row = list_bloom + (size_t)L * 256;
#pragma unroll
        for (int k = 0; k < 4; k++) row[lane + 64 * k] = 0;
    }
}

// ValidateState's order (block_validator.go:82-95): gas used where a wanted value is given, the bloom, the
// receipt root; a null want_* skips that compare.  A list that holds a failed receipt keeps that receipt's
// status, and its root row is overwritten with zeros.
__global__ __launch_bounds__(256) void k_receipt_check(const uint8_t* __restrict__ list_status, uint32_t n_lists,
                                                       const uint8_t* __restrict__ list_bloom,
                                                       uint8_t* __restrict__ root32,
                                                       const uint64_t* __restrict__ gas_used,
                                                       const uint8_t* __restrict__ want_bloom,
                                                       const uint8_t* __restrict__ want_root32,
                                                       const uint64_t* __restrict__ want_gas,
                                                       uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lists) return;
    uint32_t st = list_status[i];
    if (st != GSV_ST_OK) {
#pragma unroll 1
        for (int k = 0; k < 32; k++) root32[(size_t)i * 32 + k] = 0;
    } else if (want_gas && want_gas[i] != gas_used[i]) {
        st = GSV_ST_GAS_USED_MISMATCH;
    } else {
        uint32_t diff = 0;
        if (want_bloom) {
#pragma unroll 1
            for (int k = 0; k < 256; k++) diff |= (uint32_t)(list_bloom[(size_t)i * 256 + k] ^ want_bloom[(size_t)i * 256 + k]);
        }
        if (diff) {
            st = GSV_ST_INVALID_BLOOM;
        } else if (want_root32) {
#pragma unroll 1
            for (int k = 0; k < 32; k++) diff |= (uint32_t)(root32[(size_t)i * 32 + k] ^ want_root32[(size_t)i * 32 + k]);
            if (diff) st = GSV_ST_INVALID_RECEIPT_ROOT;
        }
    }
    status[i] = (uint8_t)st;
}

// idx_out[3 i .. 3 i + 3) = the three bit numbers of bloom9(message i)
__global__ __launch_bounds__(256) void k_bloom9(const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
                                                uint32_t n, uint16_t* __restrict__ idx_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = data + off[i];
    uint64_t len = off[i + 1] - off[i];
    uint64_t a[25], w[17];
#pragma unroll
    for (int k = 0; k < 25; k++) a[k] = 0;
    while (len >= 136) {
        load_block(w, p, 136);
#pragma unroll
        for (int k = 0; k < 17; k++) a[k] ^= w[k];
        keccakf(a);
        p += 136;
        len -= 136;
    }
    const uint32_t rem = (uint32_t)len;
    load_block(w, p, rem);
#pragma unroll
    for (int k = 0; k < 17; k++) {
        uint64_t x = w[k];
        if ((rem >> 3) == (uint32_t)k) x ^= 0x01ull << (8 * (rem & 7u));
        if (k == 16) x ^= 0x8000000000000000ULL;
        a[k] ^= x;
    }
    keccakf_digest(a);
#pragma unroll
    for (int x = 0; x < 3; x++) idx_out[(size_t)i * 3 + x] = (uint16_t)bloom_index(a[0], x);
}

static dim3 grid(uint64_t lanes) { return dim3((uint32_t)((lanes + 255) / 256)); }

hipError_t launch_receipt_scan(const uint8_t* d_vals, const uint64_t* d_voff, uint32_t n, const uint64_t* d_list_off,
                               uint32_t n_lists, uint64_t vals_bytes, uint8_t* d_work, uint8_t* d_receipt_status,
                               hipStream_t st) {
    if (n == 0) return hipSuccess;
    const rc::WorkOffsets o = rc::work_offsets(n, vals_bytes);
    hipLaunchKernelGGL(k_receipt_scan, grid(n), dim3(256), 0, st, d_vals, d_voff, n, d_list_off, n_lists, vals_bytes,
                       (uint64_t*)(d_work + o.desc), (uint64_t*)(d_work + o.gas), (uint32_t*)(d_work + o.list_idx),
                       d_receipt_status);
    return hipGetLastError();
}

hipError_t launch_receipt_bloom(const uint8_t* d_vals, const uint64_t* d_voff, uint32_t n, uint64_t vals_bytes,
                                const uint8_t* d_work, uint8_t* d_list_bloom, uint8_t* d_receipt_bloom,
                                hipStream_t st) {
    if (n == 0) return hipSuccess;
    const rc::WorkOffsets o = rc::work_offsets(n, vals_bytes);
    const uint64_t slots = rc::slot_count(vals_bytes);
    hipLaunchKernelGGL(k_receipt_bloom, dim3((uint32_t)((slots + BLOOM_WG_SLOTS - 1) / BLOOM_WG_SLOTS)), dim3(256), 0,
                       st, d_vals, d_voff, (const uint64_t*)(d_work + o.desc), slots,
                       (const uint32_t*)(d_work + o.list_idx), d_list_bloom, d_receipt_bloom);
    return hipGetLastError();
}

hipError_t launch_receipt_lists(const uint64_t* d_list_off, uint32_t n_lists, uint32_t n, uint64_t vals_bytes,
                                const uint8_t* d_work, const uint8_t* d_receipt_status, uint8_t* d_list_bloom,
                                uint64_t* d_gas_used, uint8_t* d_list_status, hipStream_t st) {
    if (n_lists == 0) return hipSuccess;
    const rc::WorkOffsets o = rc::work_offsets(n, vals_bytes);
    hipLaunchKernelGGL(k_receipt_lists, dim3((n_lists + 3) / 4), dim3(256), 0, st, d_list_off, n_lists, n,
                       d_receipt_status, (const uint64_t*)(d_work + o.gas), d_list_bloom, d_gas_used, d_list_status);
    return hipGetLastError();
}

hipError_t launch_receipt_check(const uint8_t* d_list_status, uint32_t n_lists, const uint8_t* d_list_bloom,
                                uint8_t* d_root32, const uint64_t* d_gas_used, const uint8_t* d_want_bloom,
                                const uint8_t* d_want_root32, const uint64_t* d_want_gas, uint8_t* d_status,
                                hipStream_t st) {
    if (n_lists == 0) return hipSuccess;
    hipLaunchKernelGGL(k_receipt_check, grid(n_lists), dim3(256), 0, st, d_list_status, n_lists, d_list_bloom, d_root32,
                       d_gas_used, d_want_bloom, d_want_root32, d_want_gas, d_status);
    return hipGetLastError();
}

hipError_t launch_bloom9(const uint8_t* d_data, const uint64_t* d_off, uint32_t n, uint16_t* d_idx, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bloom9, grid(n), dim3(256), 0, st, d_data, d_off, n, d_idx);
    return hipGetLastError();
}

}  // namespace gsv

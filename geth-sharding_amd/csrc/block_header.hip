// Batched Ethash.VerifyHeaders (consensus/ethash/consensus.go:90-166) without the seal: the header's RLP, its two
// hashes, and every rule of verifyHeader (consensus.go:223-285, uncle = false) around VerifySeal.
//
//   k_block_header        one header per lane: rlp.DecodeBytes into types.Header (block_header_dev.cuh), Header.Hash()
//                         and HashNoNonce() (two sponges of four or five permutations each), and a fixed-width record
//                         per header (block_header_host.h).  Lane n is the parent supplied for header 0.
//   k_block_header_rules  one header per lane: reads records i and i - 1 (the parent record for i = 0), links them by
//                         hash, runs the checks in the reference's order and writes the status in front of the seal
//                         check, the status behind it (DAO extra-data, fork hash) and the expected difficulty
//   k_block_header_merge  pre-seal status, else the seal's where it was asked for, else the post-seal status
//   k_calc_difficulty     CalcDifficulty (consensus.go:297-459) alone over decoded parents
//
// Headers link across launches (a record array between two kernels), never by waiting inside one.
#include "block_header_dev.cuh"
#include "gsv_internal.h"

namespace gsv {

using namespace bh;

namespace {

struct Records {
    uint32_t *hash, *parent_hash, *difficulty, *time;
    uint64_t *number, *gas_limit, *gas_used;
    uint32_t* flags;
};

Records records_at(uint8_t* work, size_t n) {
    const RecordOffsets o = record_offsets(n);
    return Records{(uint32_t*)(work + o.hash),       (uint32_t*)(work + o.parent_hash), (uint32_t*)(work + o.difficulty),
                   (uint32_t*)(work + o.time),       (uint64_t*)(work + o.number),      (uint64_t*)(work + o.gas_limit),
                   (uint64_t*)(work + o.gas_used),   (uint32_t*)(work + o.flags)};
}

GSV_DI void put8(uint32_t* __restrict__ rows, size_t i, const uint32_t (&w)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) rows[i * 8 + k] = w[k];
}

GSV_DI void get8(uint32_t (&w)[8], const uint32_t* __restrict__ rows, size_t i) {
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = rows[i * 8 + k];
}

}  // namespace

// Items of 2^32 bytes and more get GSV_ST_BAD_RLP unread (the host forms refuse them).  The outputs behind `rec`
// are the caller's: n rows each, null = not wanted.  hnn32 is 4-byte and nonce 8-byte aligned (what the seal
// kernels take); the other rows have any alignment.
__global__ __launch_bounds__(256) void k_block_header(const uint8_t* __restrict__ rlp, const uint64_t* __restrict__ off,
                                                      uint32_t n, const uint8_t* __restrict__ parent_rlp,
                                                      uint32_t parent_len, Records rec, uint8_t* __restrict__ hash32,
                                                      uint32_t* __restrict__ hnn32, uint64_t* __restrict__ nonce,
                                                      uint8_t* __restrict__ mix32, uint8_t* __restrict__ difficulty32,
                                                      uint64_t* __restrict__ number, uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const bool is_parent = i == n;
    const uint8_t* p = parent_rlp;
    uint64_t len64 = parent_len;
    if (!is_parent) {
        p = rlp + off[i];
        len64 = off[i + 1] - off[i];
    } else if (parent_len == 0) {
        rec.flags[i] = ST_ABSENT;
        return;
    }
    Header h;
    decode_header(h, p, len64 > 0xFFFFFFFFull ? 0u : (uint32_t)len64);
    uint32_t hash[8], hnn[8];
#pragma unroll
    for (int k = 0; k < 8; k++) hash[k] = hnn[k] = 0;
    if ((h.flags & F_STATUS) != GSV_ST_BAD_RLP) {
        const uint32_t len = (uint32_t)len64;
        keccak256_patched(hash, p, len, 0, 0);
        if (!is_parent) {
            // HashNoNonce (block.go:106-122): the first 13 fields under a list head of their own.  MixDigest and
            // Nonce are the last 42 bytes; where the shorter payload takes a shorter head the message starts one
            // byte further in
            uint64_t head_bytes;
            const uint32_t head = list_head(head_bytes, h.payload - 42);
            keccak256_patched(hnn, p + (h.head - head), head + h.payload - 42, head_bytes, head);
        }
    }
    put8(rec.hash, i, hash);
    put8(rec.parent_hash, i, h.parent_hash);
    put8(rec.difficulty, i, h.difficulty);
    put8(rec.time, i, h.time);
    rec.number[i] = h.number;
    rec.gas_limit[i] = h.gas_limit;
    rec.gas_used[i] = h.gas_used;
    rec.flags[i] = h.flags;
    if (is_parent) return;
    if (hash32) ethash::store_row32(hash32, i, hash);
    if (hnn32) put8(hnn32, i, hnn);
    if (nonce) nonce[i] = h.nonce;
    if (mix32) ethash::store_row32(mix32, i, h.mix);
    if (difficulty32) ethash::store_row32(difficulty32, i, h.difficulty);
    if (number) number[i] = h.number;
    if (status) status[i] = (uint8_t)(h.flags & F_STATUS);
}

GSV_DI Parent parent_of(const Records& rec, size_t at) {
    uint32_t d[8], t[8];
    get8(d, rec.difficulty, at);
    get8(t, rec.time, at);
    return Parent{from_row(d), from_row(t), rec.number[at], (rec.flags[at] & F_UNCLE_EMPTY) != 0};
}

// now + 15 does not wrap: now <= 2^63 (checked on the host).  want32 (null = not wanted) is the expected
// difficulty of a header that got as far as that check: zeros in front of it, 0xFF bytes for 2^256 and more.
__global__ __launch_bounds__(256) void k_block_header_rules(Records rec, uint32_t n, Config cfg, uint64_t now,
                                                            uint8_t* __restrict__ pre, uint8_t* __restrict__ post,
                                                            uint8_t* __restrict__ want32) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = i ? i - 1 : n;  // the parent's record
    const uint32_t fi = rec.flags[i], fp = rec.flags[at];
    uint32_t want[8];
#pragma unroll
    for (int k = 0; k < 8; k++) want[k] = 0;
    uint8_t st = GSV_ST_OK, st_post = GSV_ST_OK;
    uint32_t hash[8];
    get8(hash, rec.hash, i);
    const uint64_t number = rec.number[i];
    // verifyHeaderWorker (consensus.go:152-166): the parent is the header in front when its hash is ParentHash
    bool linked = (fp & F_STATUS) == GSV_ST_OK;
    if (linked) {
        uint32_t a[8], b[8], diff = 0;
        get8(a, rec.hash, at);
        get8(b, rec.parent_hash, i);
#pragma unroll
        for (int k = 0; k < 8; k++) diff |= a[k] ^ b[k];
        // chain.GetHeader(ParentHash, Number - 1), the subtraction in uint64
        linked = diff == 0 && (i != 0 || rec.number[at] == number - 1);
    }
    if ((fi & F_STATUS) != GSV_ST_OK) {
        st = (uint8_t)(fi & F_STATUS);
    } else if (!linked) {
        st = GSV_ST_UNKNOWN_ANCESTOR;
    } else {
        const Parent p = parent_of(rec, at);
        uint32_t d[8], t[8];
        get8(d, rec.difficulty, i);
        get8(t, rec.time, i);
        const U256 time = from_row(t);
        const uint64_t gas_limit = rec.gas_limit[i], parent_gas = rec.gas_limit[at];
        if ((fi >> F_EXTRA_SHIFT) > 32) {
            st = GSV_ST_EXTRA_TOO_LONG;
        } else if (!fits64(time) || low64(time) > now + 15) {
            st = GSV_ST_FUTURE_BLOCK;
        } else if (cmp(time, p.time) <= 0) {
            st = GSV_ST_ZERO_BLOCK_TIME;
        } else {
            U256 x;
            const bool over = calc_difficulty(x, cfg, low64(time), p);
            if (over) {
#pragma unroll
                for (int k = 0; k < 8; k++) want[k] = 0xFFFFFFFFu;
            } else {
                to_row(want, x);
            }
            // int64(parent.GasLimit) - int64(header.GasLimit), negated when negative: the same bits in uint64
            uint64_t gap = parent_gas - gas_limit;
            if ((int64_t)gap < 0) gap = 0 - gap;
            if (over || cmp(x, from_row(d)) != 0) st = GSV_ST_WRONG_DIFFICULTY;
            else if (gas_limit > 0x7FFFFFFFFFFFFFFFull) st = GSV_ST_GAS_LIMIT_CAP;
            else if (rec.gas_used[i] > gas_limit) st = GSV_ST_GAS_USED;
            else if (gap >= parent_gas / 1024u || gas_limit < 5000u) st = GSV_ST_GAS_LIMIT_BOUNDS;
            else if (p.number == ~0ull || number != p.number + 1) st = GSV_ST_INVALID_NUMBER;
        }
    }
    if (st == GSV_ST_OK) {
        // misc.VerifyDAOHeaderExtraData (consensus/misc/dao.go:47-69), misc.VerifyForkHashes (misc/forks.go:30-43)
        if ((cfg.flags & C_DAO) && number >= cfg.dao && number - cfg.dao < 10) {
            const bool dao_extra = (fi & F_DAO_EXTRA) != 0;
            if (cfg.flags & C_DAO_SUPPORT) st_post = dao_extra ? GSV_ST_OK : GSV_ST_BAD_PRO_DAO_EXTRA;
            else st_post = dao_extra ? GSV_ST_BAD_NO_DAO_EXTRA : GSV_ST_OK;
        }
        if (st_post == GSV_ST_OK && (cfg.flags & C_EIP150) && cfg.eip150 == number && (cfg.flags & C_EIP150_HASH)) {
            uint32_t diff = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) diff |= hash[k] ^ cfg.eip150_hash[k];
            if (diff) st_post = GSV_ST_FORK_HASH;
        }
    }
    pre[i] = st;
    post[i] = st_post;
    if (want32) ethash::store_row32(want32, i, want);
}

// seal (null: no seal was checked) holds the seal check's status per header; seals (null: all) which headers
// asked for it
__global__ __launch_bounds__(256) void k_block_header_merge(const uint8_t* __restrict__ pre,
                                                            const uint8_t* __restrict__ seal,
                                                            const uint8_t* __restrict__ seals,
                                                            const uint8_t* __restrict__ post, uint32_t n,
                                                            uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t st = pre[i];
    if (st == GSV_ST_OK && seal && (!seals || seals[i])) st = seal[i];
    if (st == GSV_ST_OK) st = post[i];
    status[i] = st;
}

__global__ __launch_bounds__(256) void k_calc_difficulty(Records rec, uint32_t n, Config cfg,
                                                         const uint64_t* __restrict__ time,
                                                         uint8_t* __restrict__ want32, uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t want[8];
#pragma unroll
    for (int k = 0; k < 8; k++) want[k] = 0;
    uint8_t st = (uint8_t)(rec.flags[i] & F_STATUS);
    if (st == GSV_ST_OK) {
        U256 x;
        if (calc_difficulty(x, cfg, time[i], parent_of(rec, i))) {
            st = GSV_ST_WRONG_DIFFICULTY;
#pragma unroll
            for (int k = 0; k < 8; k++) want[k] = 0xFFFFFFFFu;
        } else {
            to_row(want, x);
        }
    }
    ethash::store_row32(want32, i, want);
    status[i] = st;
}

static dim3 grid(uint64_t lanes) { return dim3((uint32_t)((lanes + 255) / 256)); }

hipError_t launch_block_header(const uint8_t* d_rlp, const uint64_t* d_off, uint32_t n, const uint8_t* d_parent_rlp,
                               uint32_t parent_len, uint8_t* d_work, uint8_t* d_hash32, uint8_t* d_hnn32,
                               uint64_t* d_nonce, uint8_t* d_mix32, uint8_t* d_difficulty32, uint64_t* d_number,
                               uint8_t* d_status, hipStream_t st) {
    hipLaunchKernelGGL(k_block_header, grid((uint64_t)n + 1), dim3(256), 0, st, d_rlp, d_off, n, d_parent_rlp,
                       parent_len, records_at(d_work, n), d_hash32, (uint32_t*)d_hnn32, d_nonce, d_mix32, d_difficulty32,
                       d_number, d_status);
    return hipGetLastError();
}

hipError_t launch_block_header_rules(uint8_t* d_work, uint32_t n, const bh::Config& cfg, uint64_t now, uint8_t* d_pre,
                                     uint8_t* d_post, uint8_t* d_want32, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_header_rules, grid(n), dim3(256), 0, st, records_at(d_work, n), n, cfg, now, d_pre,
                       d_post, d_want32);
    return hipGetLastError();
}

hipError_t launch_block_header_merge(const uint8_t* d_pre, const uint8_t* d_seal, const uint8_t* d_seals,
                                     const uint8_t* d_post, uint32_t n, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_block_header_merge, grid(n), dim3(256), 0, st, d_pre, d_seal, d_seals, d_post, n, d_status);
    return hipGetLastError();
}

hipError_t launch_calc_difficulty(uint8_t* d_work, uint32_t n, const bh::Config& cfg, const uint64_t* d_time,
                                  uint8_t* d_want32, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_calc_difficulty, grid(n), dim3(256), 0, st, records_at(d_work, n), n, cfg, d_time, d_want32,
                       d_status);
    return hipGetLastError();
}

}  // namespace gsv

// Host-side arithmetic of the block-header path, free of HIP (plain C++17; tests/native/block_header_host_main.cpp
// compiles it with g++): the layout of the per-header records the kernels of block_header.hip hand each other,
// the chain configuration as the kernels take it, and the compaction of the headers whose seal is still to be
// checked (gsv_block_header.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/gsv.h"

namespace gsv {
namespace bh {

// ---- the record of one decoded header, structure of arrays over m = n + 1 entries: entry i < n is header i,
// entry n the parent supplied for header 0.  Rows of 32 bytes are the byte strings as the reference holds them
// (hashes; Difficulty and Time as 32 big-endian bytes), kept as eight little-endian words.
//   hash 32 m | parent_hash 32 m | difficulty 32 m | time 32 m | number 8 m | gas_limit 8 m | gas_used 8 m | flags 4 m
// Every part starts at a multiple of 8 bytes of a 16-byte aligned work area but `flags`, at a multiple of 4.
constexpr size_t REC_BYTES = 4 * 32 + 3 * 8 + 4;

// flags word
constexpr uint32_t F_STATUS = 0xFFu;        // decode status: GSV_ST_OK, GSV_ST_BAD_RLP, GSV_ST_HEADER_TOO_WIDE, ST_ABSENT
constexpr uint32_t F_UNCLE_EMPTY = 1u << 8;  // UncleHash == types.EmptyUncleHash
constexpr uint32_t F_DAO_EXTRA = 1u << 9;    // Extra == params.DAOForkBlockExtra
constexpr uint32_t F_EXTRA_SHIFT = 16;       // len(Extra), saturating at 0xFFFF
constexpr uint32_t ST_ABSENT = 0xFFu;        // the parent entry when no parent was supplied

inline size_t work_bytes(size_t n) { return (n + 1) * REC_BYTES; }

struct RecordOffsets {
    size_t hash, parent_hash, difficulty, time, number, gas_limit, gas_used, flags, end;
};

inline RecordOffsets record_offsets(size_t n) {
    const size_t m = n + 1;
    RecordOffsets o;
    o.hash = 0;
    o.parent_hash = o.hash + 32 * m;
    o.difficulty = o.parent_hash + 32 * m;
    o.time = o.difficulty + 32 * m;
    o.number = o.time + 32 * m;
    o.gas_limit = o.number + 8 * m;
    o.gas_used = o.gas_limit + 8 * m;
    o.flags = o.gas_used + 8 * m;
    o.end = o.flags + 4 * m;
    return o;
}

// ---- the chain configuration as a kernel argument
constexpr uint32_t C_HOMESTEAD = 1, C_DAO = 2, C_EIP150 = 4, C_BYZANTIUM = 8, C_DAO_SUPPORT = 16, C_EIP150_HASH = 32;

struct Config {
    uint64_t homestead, dao, eip150, byzantium;
    uint32_t flags;
    uint32_t eip150_hash[8];  // the hash's bytes as little-endian words
};

inline Config make_config(const gsv_chain_config& g) {
    Config c;
    c.homestead = g.homestead_block;
    c.dao = g.dao_fork_block;
    c.eip150 = g.eip150_block;
    c.byzantium = g.byzantium_block;
    c.flags = (g.has_homestead ? C_HOMESTEAD : 0) | (g.has_dao_fork ? C_DAO : 0) | (g.has_eip150 ? C_EIP150 : 0) |
              (g.has_byzantium ? C_BYZANTIUM : 0) | (g.dao_fork_support ? C_DAO_SUPPORT : 0);
    uint8_t any = 0;
    for (int k = 0; k < 8; k++) {
        c.eip150_hash[k] = (uint32_t)g.eip150_hash[4 * k] | (uint32_t)g.eip150_hash[4 * k + 1] << 8 |
                           (uint32_t)g.eip150_hash[4 * k + 2] << 16 | (uint32_t)g.eip150_hash[4 * k + 3] << 24;
    }
    for (int k = 0; k < 32; k++) any |= g.eip150_hash[k];
    if (any) c.flags |= C_EIP150_HASH;  // config.EIP150Hash != (common.Hash{}) (misc/forks.go:37)
    return c;
}

// ---- the headers whose seal is checked: those the caller asked for (seals == nullptr: all) that have passed
// every rule so far.  The reference never runs VerifySeal behind an earlier failure (consensus.go:272-276).
inline void compact_sealed(const uint8_t* pre_status, const uint8_t* seals, size_t n, std::vector<uint32_t>& idx) {
    idx.clear();
    for (size_t i = 0; i < n; i++)
        if (pre_status[i] == GSV_ST_OK && (!seals || seals[i])) idx.push_back((uint32_t)i);
}

// gathers rows of `width` bytes by index
inline void gather_rows(const uint8_t* src, size_t width, const std::vector<uint32_t>& idx, std::vector<uint8_t>& out) {
    out.resize(idx.size() * width);
    for (size_t k = 0; k < idx.size(); k++) memcpy(out.data() + k * width, src + (size_t)idx[k] * width, width);
}

// the seal statuses of the compacted headers back into an array of n (zero elsewhere)
inline void scatter_status(const std::vector<uint8_t>& st, const std::vector<uint32_t>& idx, size_t n,
                           std::vector<uint8_t>& out) {
    out.assign(n, GSV_ST_OK);
    for (size_t k = 0; k < idx.size(); k++) out[idx[k]] = st[k];
}

}  // namespace bh
}  // namespace gsv

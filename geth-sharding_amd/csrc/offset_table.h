// A caller's offset table, free of HIP (plain C++17; tests/native/offset_table_main.cpp compiles it with g++).
// Every host-pointer entry point that takes variable-length items takes them packed: item i is
// data[off[i] .. off[i + 1]), off has n + 1 entries and need not start at 0.  The rule for such a table, its
// copy rebased to the first entry (what the staged copy of the bytes starts at) and the fixed-record form of
// the items exist here once.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/gsv.h"

namespace gsv {
namespace api {

constexpr uint64_t MAX_BODY = 1ull << 20;  // collationSizelimit (sharding/collation.go:45)
constexpr uint64_t MAX_POC = 1ull << 26;   // salted bodies (Proof of Custody)

// What an entry point asks of its items beyond an ascending table: the longest item it takes, and the code
// it has always returned for a table that steps backwards.
struct TableRule {
    uint64_t cap;
    int backwards;
};
// Keccak, the MD hashes, the precompiles, public keys, tx sender and tx sign: any length
constexpr TableRule kAnyLength{~0ull, GSV_E_INVALID_ARG};
// ECIES and block headers: the kernels index an item with 32 bits
constexpr TableRule kBelow4G{0xFFFFFFFFull, GSV_E_INVALID_ARG};
// chunk roots and the notary; Proof of Custody: one code for every bad entry
constexpr TableRule kBodies{MAX_BODY, GSV_E_TOO_LARGE};
constexpr TableRule kPocBodies{MAX_POC, GSV_E_TOO_LARGE};
// the blob codec's bodies: the same cap, the usual code for a backwards step
constexpr TableRule kBlobBodies{MAX_BODY, GSV_E_INVALID_ARG};

// ascending and no item above the rule's cap; only off[0 .. n] is read
inline int table_order(const uint64_t* off, size_t n, const TableRule& rule = kAnyLength) {
    for (size_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return rule.backwards;
        if (off[i + 1] - off[i] > rule.cap) return GSV_E_TOO_LARGE;
    }
    return GSV_SUCCESS;
}
// that, and a buffer behind any bytes
inline int table_check(const void* data, const uint64_t* off, size_t n, const TableRule& rule = kAnyLength) {
    const int rc = table_order(off, n, rule);
    if (rc) return rc;
    return off[n] > off[0] && !data ? GSV_E_INVALID_ARG : GSV_SUCCESS;
}

// the table rebased to its first entry, as the staged copy of the bytes is
inline std::vector<uint64_t> table_rebase(const uint64_t* off, size_t n) {
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
    return rel;
}

// common.RightPadBytes(item, rec) / getData(item, 0, rec) (core/vm/common.go:37-47) per item: out[i * rec ..)
// is the item's first `rec` bytes, zeros behind a shorter one; what follows `rec` bytes is ignored.  Writes
// exactly n * rec bytes.
inline void right_pad(const uint8_t* in, const uint64_t* off, size_t n, size_t rec, uint8_t* out) {
    memset(out, 0, n * rec);
    for (size_t i = 0; i < n; i++) {
        const size_t len = (size_t)std::min<uint64_t>(off[i + 1] - off[i], rec);
        if (len) memcpy(out + i * rec, in + off[i], len);
    }
}

}  // namespace api
}  // namespace gsv

// The work area of the receipt path, free of HIP (plain C++17; tests/native/receipt_work_main.cpp compiles it
// with g++): how many descriptor slots a batch of vals_bytes bytes of receipt RLP takes, and where the three
// arrays that receipt.hip's kernels hand each other lie in the caller's d_work.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gsv {
namespace rc {

// A bloom item (a log's address or one of its topics) takes at least 21 bytes of RLP: 0x94 and 20 bytes, or
// 0xa0 and 32.  So two items' head bytes are at least 21 apart, and position / 21 is a slot of its own.
constexpr uint32_t SLOT_BYTES = 21;
// the receipts of one call: fewer than 2^31 of them, at most 2^40 bytes (a grid of 2^40 / 21 / 2048 workgroups)
constexpr uint64_t MAX_RECEIPTS = 0x7FFFFFFFull;
constexpr uint64_t MAX_VALS_BYTES = 1ull << 40;

// slots of the descriptor table: every position in [0, vals_bytes) has one
inline uint64_t slot_count(uint64_t vals_bytes) { return vals_bytes / SLOT_BYTES + 1; }

// d_work (8-byte aligned): descriptors 8 x slots | CumulativeGasUsed 8 n | list index 4 n, padded to 8
struct WorkOffsets {
    size_t desc, gas, list_idx, total;
};

inline WorkOffsets work_offsets(size_t n, uint64_t vals_bytes) {
    WorkOffsets o;
    o.desc = 0;
    o.gas = (size_t)slot_count(vals_bytes) * 8;
    o.list_idx = o.gas + n * 8;
    o.total = (o.list_idx + n * 4 + 7) & ~(size_t)7;
    return o;
}

// 0 for a batch past the two bounds above (the entry points refuse it)
inline size_t work_bytes(size_t n, uint64_t vals_bytes) {
    if (n > MAX_RECEIPTS || vals_bytes > MAX_VALS_BYTES) return 0;
    return work_offsets(n, vals_bytes).total;
}

}  // namespace rc
}  // namespace gsv

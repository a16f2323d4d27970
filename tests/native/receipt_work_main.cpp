// Stand-alone check of csrc/receipt_host.h (g++, with ASan + UBSan when the compiler links them): the descriptor
// table has a slot of its own for every bloom item, whatever the items' positions, and the three arrays of the
// work area neither overlap nor pass its end.  Items are laid out the way k_receipt_scan places them (slot =
// position / 21) into a table of exactly slot_count entries on the heap, so a slot past the end is a sanitizer
// error and two items in one slot are counted.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../geth-sharding_amd/csrc/receipt_host.h"

using namespace gsv::rc;

static int fails = 0;
#define CHECK(x)                                             \
    do {                                                     \
        if (!(x)) {                                          \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
            fails++;                                         \
        }                                                    \
    } while (0)

// items of 21 (address) or 33 (topic) bytes of RLP packed back to back from `start`, with `gap` bytes between
static void pack(uint64_t vals_bytes, uint64_t start, uint64_t gap, unsigned pattern) {
    std::vector<uint64_t> table(slot_count(vals_bytes), 0);
    uint64_t at = start, items = 0;
    while (true) {
        const uint64_t len = (pattern >> (items % 8)) & 1 ? 33 : 21;
        if (at + len > vals_bytes) break;  // an item lies inside the receipts' bytes
        uint64_t& slot = table.at(at / SLOT_BYTES);
        CHECK(slot == 0);
        slot = 1 + at % SLOT_BYTES;
        CHECK(at / SLOT_BYTES * SLOT_BYTES + (slot - 1) == at);  // the position comes back from slot and remainder
        at += len + gap;
        items++;
    }
    uint64_t used = 0;
    for (uint64_t s : table) used += s != 0;
    CHECK(used == items);
}

int main() {
    CHECK(SLOT_BYTES == 21);
    CHECK(slot_count(0) == 1 && slot_count(20) == 1 && slot_count(21) == 2 && slot_count(2100) == 101);
    for (uint64_t bytes : {0ull, 1ull, 20ull, 21ull, 22ull, 41ull, 42ull, 43ull, 1000ull, 4099ull})
        for (uint64_t start = 0; start < 23; start++)
            for (uint64_t gap : {0ull, 1ull, 2ull, 20ull})
                for (unsigned pattern : {0x00u, 0xFFu, 0x55u, 0x0Fu}) pack(bytes, start, gap, pattern);
    // the last byte of the batch has a slot
    for (uint64_t bytes = 1; bytes < 200; bytes++) CHECK((bytes - 1) / SLOT_BYTES < slot_count(bytes));
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)1000})
        for (uint64_t bytes : {0ull, 20ull, 21ull, 2100ull, 1ull << 20}) {
            const WorkOffsets o = work_offsets(n, bytes);
            CHECK(o.desc == 0 && o.gas == slot_count(bytes) * 8 && o.list_idx == o.gas + 8 * n);
            CHECK(o.total >= o.list_idx + 4 * n && o.total < o.list_idx + 4 * n + 8 && o.total % 8 == 0);
            CHECK(o.gas % 8 == 0 && o.list_idx % 4 == 0);
            CHECK(work_bytes(n, bytes) == o.total);
        }
    CHECK(work_bytes(MAX_RECEIPTS, 0) != 0 && work_bytes(MAX_RECEIPTS + 1, 0) == 0);
    CHECK(work_bytes(1, MAX_VALS_BYTES) != 0 && work_bytes(1, MAX_VALS_BYTES + 1) == 0);
    // the largest call: no wrap in 64 bits
    const WorkOffsets big = work_offsets(MAX_RECEIPTS, MAX_VALS_BYTES);
    CHECK(big.total > big.list_idx && big.list_idx > big.gas && big.gas == (MAX_VALS_BYTES / 21 + 1) * 8);
    if (fails) return 1;
    printf("ok receipt work area\n");
    return 0;
}

// Stand-alone check of csrc/offset_table.h: the rule for a caller's offset table under each entry point's
// TableRule (with the code that entry point returns), the rebased copy, and the fixed-record form of the
// items.  Only offsets are read by the table checks, so the items of 2^32 and 2^33 bytes need no buffer.
// Meant to be compiled with ASan + UBSan and run as a child process.  Prints "ok <checks>" and exits 0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../geth-sharding_amd/csrc/offset_table.h"

using namespace gsv::api;

static int g_fail = 0, g_checks = 0;

#define EXPECT(cond, ...)          \
    do {                           \
        g_checks++;                \
        if (!(cond)) {             \
            printf("FAIL ");       \
            printf(__VA_ARGS__);   \
            printf("\n");          \
            g_fail++;              \
        }                          \
    } while (0)

struct NamedRule {
    const char* name;
    TableRule rule;
    int backwards;  // what the entry points under this rule return for a table that steps backwards
};

int main() {
    static const uint8_t kData[1] = {0};  // never read by the table checks
    const NamedRule rules[] = {
        {"any length (Keccak, MD hashes, precompiles, keys, tx sender, tx sign)", kAnyLength, GSV_E_INVALID_ARG},
        {"below 2^32 (ECIES, block headers)", kBelow4G, GSV_E_INVALID_ARG},
        {"MAX_BODY (chunk roots, notary)", kBodies, GSV_E_TOO_LARGE},
        {"MAX_POC (Proof of Custody)", kPocBodies, GSV_E_TOO_LARGE},
        {"MAX_BODY (blob codec)", kBlobBodies, GSV_E_INVALID_ARG},
    };
    EXPECT(kBelow4G.cap == 0xFFFFFFFFull && kBodies.cap == (1ull << 20) && kPocBodies.cap == (1ull << 26) &&
               kBlobBodies.cap == kBodies.cap,
           "the caps in use");
    for (const NamedRule& r : rules) {
        for (uint64_t base : {(uint64_t)0, (uint64_t)5}) {
            // n = 1 and n = 3, ascending, from a zero and a nonzero first entry
            const uint64_t one[2] = {base, base + 9};
            const uint64_t three[4] = {base, base + 4, base + 4, base + 10};
            EXPECT(table_check(kData, one, 1, r.rule) == GSV_SUCCESS, "%s: n=1 base=%llu", r.name,
                   (unsigned long long)base);
            EXPECT(table_check(kData, three, 3, r.rule) == GSV_SUCCESS, "%s: n=3 base=%llu", r.name,
                   (unsigned long long)base);
            EXPECT(table_order(three, 3, r.rule) == GSV_SUCCESS, "%s: order n=3", r.name);
            // a non-empty table needs a data pointer, an all-empty one does not
            EXPECT(table_check(nullptr, three, 3, r.rule) == GSV_E_INVALID_ARG, "%s: bytes without a buffer", r.name);
            const uint64_t empty[4] = {base, base, base, base};
            EXPECT(table_check(nullptr, empty, 3, r.rule) == GSV_SUCCESS, "%s: all-empty table, null data", r.name);
            EXPECT(table_check(nullptr, empty, 1, r.rule) == GSV_SUCCESS, "%s: one empty item, null data", r.name);
            // a step backwards at the first, middle and last entry (and the only entry of n = 1)
            for (int at = 0; at < 3; at++) {
                uint64_t t[4] = {base + 10, base + 20, base + 30, base + 40};
                t[at + 1] = t[at] - 1;
                if (at < 2) t[at + 2] = t[at + 1] + 1;  // the rest ascends again: only one step is wrong
                if (at == 0) t[3] = t[2] + 1;
                EXPECT(table_check(kData, t, 3, r.rule) == r.backwards, "%s: backwards at entry %d", r.name, at);
                EXPECT(table_order(t, 3, r.rule) == r.backwards, "%s: order, backwards at entry %d", r.name, at);
            }
            const uint64_t back1[2] = {base + 3, base + 2};
            EXPECT(table_check(kData, back1, 1, r.rule) == r.backwards, "%s: n=1 backwards", r.name);
            // an item of exactly the cap, and of one byte more, at each position of n = 3
            if (r.rule.cap != ~0ull)
                for (int at = 0; at < 3; at++) {
                    uint64_t t[4] = {base, base + 1, base + 2, base + 3};
                    for (int k = at + 1; k < 4; k++) t[k] += r.rule.cap - 1;
                    EXPECT(table_check(kData, t, 3, r.rule) == GSV_SUCCESS, "%s: an item of the cap at %d", r.name, at);
                    for (int k = at + 1; k < 4; k++) t[k] += 1;
                    EXPECT(table_check(kData, t, 3, r.rule) == GSV_E_TOO_LARGE, "%s: cap + 1 at %d", r.name, at);
                    EXPECT(table_check(nullptr, t, 3, r.rule) == GSV_E_TOO_LARGE, "%s: cap + 1 before the data check",
                           r.name);
                }
        }
    }
    // the uncapped mode takes an item of 2^33 bytes; the 32-bit rule takes 2^32 - 1 and refuses 2^32
    const uint64_t huge[3] = {7, 7 + (1ull << 33), 8 + (1ull << 33)};
    EXPECT(table_check(kData, huge, 2) == GSV_SUCCESS, "default rule: 2^33-byte item");
    EXPECT(table_check(kData, huge, 2, kAnyLength) == GSV_SUCCESS, "any length: 2^33-byte item");
    EXPECT(table_check(kData, huge, 2, kBelow4G) == GSV_E_TOO_LARGE, "below 2^32: 2^33-byte item");
    const uint64_t edge[2] = {3, 3 + 0xFFFFFFFFull}, over[2] = {3, 3 + (1ull << 32)};
    EXPECT(table_check(kData, edge, 1, kBelow4G) == GSV_SUCCESS, "below 2^32: 2^32 - 1 bytes");
    EXPECT(table_check(kData, over, 1, kBelow4G) == GSV_E_TOO_LARGE, "below 2^32: 2^32 bytes");
    // a backwards step in front of an oversized item is reported first (the entry points' order)
    const uint64_t both[4] = {9, 8, 8, 8 + (1ull << 33)};
    EXPECT(table_check(kData, both, 3, kBelow4G) == GSV_E_INVALID_ARG, "backwards before too large");
    const uint64_t both2[4] = {0, 1ull << 33, 5, 6};
    EXPECT(table_check(kData, both2, 3, kBelow4G) == GSV_E_TOO_LARGE, "too large before backwards");

    // ---- rebase
    for (uint64_t base : {(uint64_t)0, (uint64_t)7}) {
        const uint64_t t[4] = {base, base + 3, base + 3, base + 300};
        for (size_t n : {(size_t)1, (size_t)3}) {
            const std::vector<uint64_t> rel = table_rebase(t, n);
            EXPECT(rel.size() == n + 1 && rel[0] == 0, "rebase: n + 1 entries from 0 (base %llu)", (unsigned long long)base);
            for (size_t i = 0; i < n && i + 1 < rel.size(); i++)
                EXPECT(rel[i + 1] - rel[i] == t[i + 1] - t[i], "rebase: item %zu keeps its length", i);
        }
    }

    // ---- right-pad: item lengths 0, rec - 1, rec, rec + 1 behind a prefix the table skips
    for (size_t rec : {(size_t)96, (size_t)128}) {
        const size_t lens[4] = {0, rec - 1, rec, rec + 1}, n = 4, base = 3;
        std::vector<uint8_t> in(base, 0xEE);
        uint64_t off[5];
        off[0] = base;
        for (size_t i = 0; i < n; i++) {
            for (size_t k = 0; k < lens[i]; k++) in.push_back((uint8_t)(1 + (i * 37 + k) % 250));  // never zero
            off[i + 1] = in.size();
        }
        std::vector<uint8_t> buf(1 + n * rec + 1, 0xCC);  // a guard byte on either side
        right_pad(in.data(), off, n, rec, buf.data() + 1);
        EXPECT(buf.front() == 0xCC && buf.back() == 0xCC, "right_pad rec=%zu: writes n * rec bytes exactly", rec);
        for (size_t i = 0; i < n; i++) {
            const size_t kept = lens[i] < rec ? lens[i] : rec;
            const uint8_t* row = buf.data() + 1 + i * rec;
            EXPECT(kept == 0 || memcmp(row, in.data() + off[i], kept) == 0, "right_pad rec=%zu: item %zu's bytes", rec, i);
            bool zero = true;
            for (size_t k = kept; k < rec; k++) zero = zero && row[k] == 0;
            EXPECT(zero, "right_pad rec=%zu: item %zu padded with zeros", rec, i);
        }
        // n = 1, and an empty item with no buffer at all
        std::vector<uint8_t> one(1 + rec + 1, 0xCC);
        const uint64_t none[2] = {5, 5};
        right_pad(nullptr, none, 1, rec, one.data() + 1);
        bool zero = one.front() == 0xCC && one.back() == 0xCC;
        for (size_t k = 0; k < rec; k++) zero = zero && one[1 + k] == 0;
        EXPECT(zero, "right_pad rec=%zu: an empty item is all padding", rec);
    }
    if (g_fail) {
        printf("%d failure(s)\n", g_fail);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}

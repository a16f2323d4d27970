// Host arithmetic of the bloombits family, free of HIP (plain C++17; tests/native/bloombits_host_main.cpp compiles
// it with g++): the bounds of a call and the sizes of its arrays, NewMatcher's dropping of rules, and the packing
// of compressed slots into one byte string behind an offset table.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace gsv {
namespace bb {

constexpr uint32_t BLOOM_BYTES = 256, BLOOM_BITS = 2048;
constexpr uint32_t MIN_SECTION = 8, MAX_SECTION = 32768;  // include/gsv.h: GSV_BLOOMBITS_MAX_SECTION
constexpr uint32_t MAX_VECTOR = 4096;                     // GSV_BITSET_MAX_LEN
constexpr uint64_t MAX_SECTIONS = 1ull << 20, MAX_QUERIES = 1ull << 20, MAX_RULES = 1ull << 20,
                   MAX_CLAUSES = 1ull << 20, MAX_PAIRS = 1ull << 24, MAX_VECTORS = 0x7FFFFFFFull;
constexpr uint64_t MAX_BLOOMS = 1ull << 31;

// generator.go:40 and our two bounds
inline bool section_ok(uint64_t s) { return s >= MIN_SECTION && s <= MAX_SECTION && s % 8 == 0; }
inline uint64_t row_bytes(uint32_t s) { return s / 8; }
// the table of n sections: at most 2^20 x 2048 x 4096 = 2^43 bytes, no wrap in 64 bits
inline uint64_t table_bytes(uint64_t n_sections, uint32_t s) { return n_sections * BLOOM_BITS * row_bytes(s); }
inline uint64_t blooms_bytes(uint64_t n_sections, uint32_t s) { return n_sections * s * BLOOM_BYTES; }
// the match bitsets of a call: 0 past the bound on (query, section) pairs
inline uint64_t match_bytes(uint64_t n_queries, uint64_t n_sections, uint32_t s) {
    if (n_queries > MAX_QUERIES || n_sections > MAX_SECTIONS || n_queries * n_sections > MAX_PAIRS) return 0;
    return n_queries * n_sections * row_bytes(s);
}
inline bool pairs_ok(uint64_t n_queries, uint64_t n_sections) {
    return n_queries <= MAX_QUERIES && n_sections <= MAX_SECTIONS && n_queries * n_sections <= MAX_PAIRS;
}

// The filter system NewMatcher keeps (matcher.go:105-122) of the one it is given: a rule with no clauses is
// dropped (:107-109), a rule with a nil clause is dropped (:112-115, :119-121), every other rule keeps its clauses
// in order.  In: query q holds rules [query_off[q], query_off[q+1]), rule r clauses [rule_off[r], rule_off[r+1]),
// nil[c] != 0 marks a nil clause (nil == nullptr: none).  Out: the same two tables over the rules and clauses that
// remain, and for each kept clause its index in the input (what is hashed).  False: a table steps backwards.
struct Filters {
    std::vector<uint32_t> query_off, rule_off;
    std::vector<uint64_t> clause;  // input index of kept clause k
};

inline bool drop_rules(const uint64_t* query_off, size_t n_queries, const uint64_t* rule_off, const uint8_t* nil,
                       Filters& f) {
    f.query_off.assign(1, 0);
    f.rule_off.assign(1, 0);
    f.clause.clear();
    for (size_t q = 0; q < n_queries; q++) {
        if (query_off[q + 1] < query_off[q]) return false;
        for (uint64_t r = query_off[q]; r < query_off[q + 1]; r++) {
            if (rule_off[r + 1] < rule_off[r]) return false;
            bool keep = rule_off[r + 1] > rule_off[r];
            for (uint64_t c = rule_off[r]; keep && c < rule_off[r + 1]; c++) keep = !(nil && nil[c]);
            if (!keep) continue;
            for (uint64_t c = rule_off[r]; c < rule_off[r + 1]; c++) f.clause.push_back(c);
            f.rule_off.push_back((uint32_t)f.clause.size());
        }
        f.query_off.push_back((uint32_t)(f.rule_off.size() - 1));
    }
    return true;
}

// The compressed slots of n vectors of length L (slot i = slots[i L ..), len[i] bytes of it) packed back to back:
// off[0] = 0, off[i + 1] = off[i] + len[i], out[off[i] ..) = the slot's bytes.  False, with nothing past out[n L)
// written, when a length exceeds L (never from the kernel).  out may be the slots' own memory: the packing moves
// bytes towards the front only.
inline bool pack_slots(const uint8_t* slots, const uint32_t* len, size_t n, uint32_t L, uint8_t* out, uint64_t* off) {
    off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (len[i] > L) return false;
        if (len[i]) memmove(out + off[i], slots + i * (size_t)L, len[i]);
        off[i + 1] = off[i] + len[i];
    }
    return true;
}

}  // namespace bb
}  // namespace gsv

// Stand-alone check of csrc/bloombits_host.h (g++, with ASan + UBSan when the compiler links them): NewMatcher's
// dropping of rules over every combination of empty / nil / plain clauses in up to three rules, the packing of
// compressed slots behind an offset table, and the size arithmetic at the bounds of S and at sizes past 32 bits.
// Every table lives in a heap vector of exactly its length, so a read or write past an end is a sanitizer error.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../geth-sharding_amd/csrc/bloombits_host.h"

using namespace gsv::bb;

static int fails = 0;
#define CHECK(x)                                               \
    do {                                                       \
        if (!(x)) {                                            \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x); \
            fails++;                                           \
        }                                                      \
    } while (0)

// a rule's shape: its clauses, each plain (0), empty but not nil (1) or nil (2); -1 clauses: a nil rule (no clauses)
struct Rule {
    std::vector<int> kinds;
};

// the reference's loop (matcher.go:105-122) over the shapes, stated on its own: which rules stay
static std::vector<std::vector<int>> reference_keep(const std::vector<Rule>& rules) {
    std::vector<std::vector<int>> out;
    for (const Rule& r : rules) {
        if (r.kinds.empty()) continue;
        bool nil = false;
        for (int k : r.kinds) nil = nil || k == 2;
        if (!nil) out.push_back(r.kinds);
    }
    return out;
}

static void check_query(const std::vector<Rule>& rules, uint64_t first_rule, uint64_t first_clause) {
    // tables that do not start at 0: rule_off is indexed by the query table's entries, nil by the rule table's
    std::vector<uint64_t> query_off{first_rule, first_rule + rules.size()};
    std::vector<uint64_t> rule_off(first_rule + rules.size() + 1, first_clause);
    std::vector<uint8_t> nil(first_clause, 1);  // what lies in front is nil: it must never be looked at
    std::vector<int> kind_of(first_clause, -1);
    for (size_t r = 0; r < rules.size(); r++) {
        for (int k : rules[r].kinds) {
            nil.push_back(k == 2);
            kind_of.push_back(k);
        }
        rule_off[first_rule + r + 1] = nil.size();
    }
    Filters f;
    CHECK(drop_rules(query_off.data(), 1, rule_off.data(), nil.data(), f));
    const auto want = reference_keep(rules);
    CHECK(f.query_off.size() == 2 && f.query_off[0] == 0 && f.query_off[1] == want.size());
    CHECK(f.rule_off.size() == want.size() + 1 && f.rule_off[0] == 0);
    size_t at = 0;
    for (size_t r = 0; r < want.size() && r + 1 < f.rule_off.size(); r++) {
        CHECK(f.rule_off[r + 1] - f.rule_off[r] == want[r].size());
        for (int k : want[r]) {
            CHECK(at < f.clause.size() && f.clause[at] >= first_clause && kind_of.at(f.clause[at]) == k);
            at++;
        }
    }
    CHECK(at == f.clause.size());
    for (size_t k = 1; k < f.clause.size(); k++) CHECK(f.clause[k] > f.clause[k - 1]);  // the input's order
    // nil == nullptr: only the rules without clauses go
    Filters g;
    CHECK(drop_rules(query_off.data(), 1, rule_off.data(), nullptr, g));
    size_t nonempty = 0;
    for (const Rule& r : rules) nonempty += !r.kinds.empty();
    CHECK(g.rule_off.size() == nonempty + 1);
}

static void dropping() {
    // every rule of 0, 1 or 2 clauses over the three kinds: 1 + 3 + 9 = 13 shapes; every query of up to 3 rules
    std::vector<Rule> shapes;
    shapes.push_back({{}});
    for (int a = 0; a < 3; a++) shapes.push_back({{a}});
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) shapes.push_back({{a, b}});
    const size_t n = shapes.size();
    size_t queries = 0;
    check_query({}, 0, 0);
    for (size_t a = 0; a < n; a++) {
        check_query({shapes[a]}, 0, 0);
        check_query({shapes[a]}, 3, 5);
        for (size_t b = 0; b < n; b++) {
            check_query({shapes[a], shapes[b]}, 0, 0);
            for (size_t c = 0; c < n; c++) {
                check_query({shapes[a], shapes[b], shapes[c]}, (a + b + c) % 3, (a * b + c) % 4);
                queries++;
            }
        }
    }
    CHECK(queries == 13 * 13 * 13);
    // TestMatcherWildcards' eight rules in one query: three stay, of 2, 2 and 1 clauses
    check_query({{{0, 0}}, {{0, 0}}, {{0}}, {{0, 2}}, {{2, 0}}, {{2, 2}}, {{}}, {{}}}, 0, 0);
    // several queries, one without rules; and tables that step backwards
    {
        std::vector<uint64_t> query_off{0, 2, 2, 3}, rule_off{0, 1, 1, 3};
        std::vector<uint8_t> nil{0, 0, 1};
        Filters f;
        CHECK(drop_rules(query_off.data(), 3, rule_off.data(), nil.data(), f));
        CHECK((f.query_off == std::vector<uint32_t>{0, 1, 1, 1}) && (f.rule_off == std::vector<uint32_t>{0, 1}));
        CHECK(f.clause == std::vector<uint64_t>{0});
        std::vector<uint64_t> qback{0, 2, 1}, rback{0, 2, 1};
        CHECK(!drop_rules(qback.data(), 2, rule_off.data(), nullptr, f));
        CHECK(!drop_rules(query_off.data(), 1, rback.data(), nullptr, f));
    }
}

static void packing() {
    for (uint32_t L : {1u, 2u, 9u, 512u, 4096u})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)64}) {
            std::vector<uint8_t> slots(n * L + 1, 0xEE);
            std::vector<uint32_t> len(n);
            std::vector<uint8_t> want;
            for (size_t i = 0; i < n; i++) {
                len[i] = i % 4 == 0 ? 0 : i % 4 == 1 ? L : i % 4 == 2 ? (L + 1) / 2 : L - 1;
                for (uint32_t k = 0; k < len[i]; k++) {
                    slots[i * L + k] = (uint8_t)(1 + (i * 7 + k) % 250);
                    want.push_back(slots[i * L + k]);
                }
            }
            // into a buffer of its own of exactly the packed size, and in place
            std::vector<uint8_t> out(want.size() + 1, 0xDD);
            std::vector<uint64_t> off(n + 1, 99);
            CHECK(pack_slots(slots.data(), len.data(), n, L, out.data(), off.data()));
            CHECK(off[0] == 0 && off[n] == want.size() && out[want.size()] == 0xDD);
            for (size_t i = 0; i < n; i++) CHECK(off[i + 1] - off[i] == len[i]);
            CHECK(std::vector<uint8_t>(out.begin(), out.end() - 1) == want);
            CHECK(pack_slots(slots.data(), len.data(), n, L, slots.data(), off.data()));
            CHECK(std::vector<uint8_t>(slots.begin(), slots.begin() + want.size()) == want && slots[n * L] == 0xEE);
            if (n) {
                len[n - 1] = L + 1;  // never from the kernel: refused, nothing written past the slots
                CHECK(!pack_slots(slots.data(), len.data(), n, L, slots.data(), off.data()));
                CHECK(slots[n * L] == 0xEE);
            }
        }
}

static void sizes() {
    for (uint64_t s : {0ull, 1ull, 4ull, 7ull, 9ull, 12ull, 32769ull, 32776ull, 65536ull, 1ull << 32, (1ull << 32) + 8})
        CHECK(!section_ok(s));
    for (uint64_t s : {8ull, 16ull, 72ull, 2048ull, 4096ull, 32760ull, 32768ull}) CHECK(section_ok(s));
    CHECK(row_bytes(8) == 1 && row_bytes(72) == 9 && row_bytes(32768) == 4096 && MAX_VECTOR == 4096);
    CHECK(table_bytes(1, 8) == 2048 && table_bytes(3, 72) == 3ull * 2048 * 9 && blooms_bytes(3, 72) == 3ull * 72 * 256);
    CHECK(table_bytes(1, 4096) == 1ull << 20 && blooms_bytes(1, 4096) == 1ull << 20);  // a section in = a section out
    // past 32 bits: 4,097 sections of 4,096 are 2^32 + 2^20 bytes; the largest call is 2^43
    CHECK(table_bytes(4097, 4096) == (1ull << 32) + (1ull << 20) && blooms_bytes(4097, 4096) == table_bytes(4097, 4096));
    CHECK(table_bytes(MAX_SECTIONS, MAX_SECTION) == 1ull << 43 && blooms_bytes(MAX_SECTIONS, MAX_SECTION) == 1ull << 43);
    CHECK(match_bytes(1024, 1221, 4096) == 1024ull * 1221 * 512);
    CHECK(match_bytes(1 << 12, 1 << 12, 32768) == 1ull << 36 && pairs_ok(1 << 12, 1 << 12));  // 2^24 pairs of 4 KiB
    CHECK(match_bytes((1 << 12) + 1, 1 << 12, 8) == 0 && !pairs_ok((1 << 12) + 1, 1 << 12));
    CHECK(match_bytes(MAX_QUERIES + 1, 1, 8) == 0 && match_bytes(1, MAX_SECTIONS + 1, 8) == 0);
    CHECK(match_bytes(1ull << 40, 1ull << 40, 8) == 0);  // the product wraps; each factor is refused first
    CHECK(match_bytes(0, 5, 8) == 0 && pairs_ok(0, 5) && match_bytes(MAX_QUERIES, 16, 8) == MAX_QUERIES * 16);
}

int main() {
    dropping();
    packing();
    sizes();
    if (fails) return 1;
    printf("ok bloombits host arithmetic\n");
    return 0;
}

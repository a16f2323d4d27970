// csrc/ethash_host.h's seal_round as a stand-alone program (tests/test_ethash_full_cpu.py builds it with
// g++ -fsanitize=address,undefined and runs it): the sizing of the sealer's rounds, and a replay of
// gsv_ethash_seal_batch's bookkeeping over it (how many nonces each header has been given when the rounds end).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../geth-sharding_amd/csrc/ethash_host.h"

namespace eth = gsv::ethash;

static int fails = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #x);    \
            fails++;                                              \
        }                                                         \
    } while (0)

int main() {
    // nothing to do
    CHECK(eth::seal_round(0, 100).headers == 0 && eth::seal_round(0, 100).span == 0);
    CHECK(eth::seal_round(5, 0).headers == 0 && eth::seal_round(5, 0).span == 0);

    const uint64_t counts[] = {1, 2, 3, 7, 8, 255, 256, 257, 1000, 16383, 16384, 16385, 100000, 0x7FFFFFFFull};
    const uint64_t lefts[] = {1, 2, 255, 256, 257, 1000, 8192, 1ull << 22, (1ull << 22) + 1, 1ull << 40, ~0ull};
    for (uint64_t m : counts)
        for (uint64_t left : lefts) {
            const eth::SealRound r = eth::seal_round(m, left);
            CHECK(r.headers >= 1 && r.headers <= m);
            CHECK(r.span >= 1 && r.span <= left);                  // progress, and never past the caller's bound
            CHECK(r.span <= 0xFFFFFFFFull);                        // the search's offsets are 32 bits
            CHECK(r.headers * r.span <= eth::SEAL_ROUND_ITEMS);    // a launch of milliseconds
            CHECK(r.span == left || r.span % eth::SEAL_BLOCK == 0);  // whole workgroups unless the bound cuts it
            // as much as the round may hold: either every header, or a full round of 256-nonce slices
            CHECK(r.headers == m || r.headers * eth::SEAL_BLOCK == eth::SEAL_ROUND_ITEMS);
            // the grid of gsv_ethash_search_dev: headers * ceil(span / 256) workgroups
            CHECK(r.headers * ((r.span + 255) / 256) <= 0x7FFFFFFFull);
        }
    CHECK(eth::seal_round(1, ~0ull).span == eth::SEAL_ROUND_ITEMS);
    CHECK(eth::seal_round(8, 8192).span == 8192 && eth::seal_round(8, 8192).headers == 8);
    CHECK(eth::seal_round(16384, 1024).span == 256 && eth::seal_round(16384, 1024).headers == 16384);
    CHECK(eth::seal_round(16385, 1024).span == 256 && eth::seal_round(16385, 1024).headers == 16384);

    // the rounds of one epoch group where nobody is ever found: every header is tried exactly max_attempts times
    for (uint64_t m : {1ull, 9ull, 16384ull, 40000ull})
        for (uint64_t max_attempts : {1ull, 300ull, 1024ull, (1ull << 23) + 5}) {
            uint64_t tried = 0, rounds = 0;
            while (tried < max_attempts) {
                const eth::SealRound r = eth::seal_round(m, max_attempts - tried);
                if (r.span == 0) break;
                uint64_t covered = 0;
                for (uint64_t at = 0; at < m; at += r.headers) covered += (m - at < r.headers ? m - at : r.headers);
                CHECK(covered == m);
                tried += r.span;
                rounds++;
            }
            CHECK(tried == max_attempts && rounds >= 1);
        }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}

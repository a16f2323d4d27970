// csrc/ethash_host.h and csrc/ethash_mod.h as a stand-alone program (tests/test_ethash_cpu.py builds it with
// ASan + UBSan and runs it as a child process).  Its argument is a text file of fixture rows:
//
//   size <block> <cache size> <dataset size> <seed hex>
//   sizes_digest <Keccak-256 of the 2,048 cache sizes as LE u64> <the same of the dataset sizes>
//   small_cache <block> <bytes> <hex of the whole cache>          generated from seed_hash(block)
//   full_cache <block> <digest hex>                               cache_size(block) bytes from seed_hash(block)
//   full_row <row> <hex of the 64 bytes>                          of the full_cache before it
//
// and it checks the reciprocal reduction against % on its own.  Prints "ok", or the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/ethash_host.h"

namespace eth = gsv::ethash;

static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s += d[p[i] >> 4];
        s += d[p[i] & 15];
    }
    return s;
}

static int fail(const std::string& what) {
    std::cout << "mismatch: " << what << "\n";
    return 1;
}

static bool check_mod(uint32_t rows) {
    const eth::ModRecip r = eth::mod_recip(rows);
    auto one = [&](uint64_t x) {
        if (x > 0xFFFFFFFFull) return true;
        return eth::mod_reduce((uint32_t)x, r) == (uint32_t)x % rows;
    };
    bool ok = one(0) && one(1) && one(1ull << 31) && one(0xFFFFFFFFull);
    const uint64_t ks[3] = {1, 2, 0xFFFFFFFFull / rows};
    for (uint64_t k : ks) ok = ok && one(k * rows - 1) && one(k * rows) && one(k * rows + 1);
    std::mt19937_64 rng(0x65746861ull ^ rows);
    for (int i = 0; i < 1000000 && ok; i++) ok = one((uint32_t)rng());
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    std::vector<uint8_t> full;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string key;
        ls >> key;
        if (key == "size") {
            uint64_t block, cs, ds;
            std::string seed;
            ls >> block >> cs >> ds >> seed;
            uint8_t s[32];
            eth::seed_hash(block, s);
            if (eth::cache_size(block) != cs || eth::dataset_size(block) != ds || hex(s, 32) != seed)
                return fail("sizes or seed of block " + std::to_string(block));
        } else if (key == "sizes_digest") {
            std::string want_c, want_d;
            ls >> want_c >> want_d;
            std::vector<uint8_t> cs(2048 * 8), ds(2048 * 8);
            for (uint64_t e = 0; e < 2048; e++) {
                eth::store_le64(&cs[e * 8], eth::calc_cache_size(e));
                eth::store_le64(&ds[e * 8], eth::calc_dataset_size(e));
            }
            uint8_t d[32];
            eth::keccak256(d, cs.data(), cs.size());
            if (hex(d, 32) != want_c) return fail("the 2,048 cache sizes");
            eth::keccak256(d, ds.data(), ds.size());
            if (hex(d, 32) != want_d) return fail("the 2,048 dataset sizes");
        } else if (key == "small_cache") {
            uint64_t block, bytes;
            std::string want;
            ls >> block >> bytes >> want;
            uint8_t s[32];
            eth::seed_hash(block, s);
            std::vector<uint8_t> c(bytes);
            if (!eth::make_cache(s, bytes, c.data()) || hex(c.data(), bytes) != want)
                return fail("small cache of block " + std::to_string(block));
        } else if (key == "full_cache") {
            uint64_t block;
            std::string want;
            ls >> block >> want;
            uint8_t s[32], d[32];
            eth::seed_hash(block, s);
            full.assign(eth::cache_size(block), 0);
            if (!eth::make_cache(s, full.size(), full.data())) return fail("make_cache");
            eth::keccak256(d, full.data(), full.size());
            if (hex(d, 32) != want) return fail("digest of the full cache of block " + std::to_string(block));
        } else if (key == "full_row") {
            uint64_t row;
            std::string want;
            ls >> row >> want;
            if ((row + 1) * 64 > full.size() || hex(&full[row * 64], 64) != want)
                return fail("row " + std::to_string(row) + " of the full cache");
        } else if (!key.empty()) {
            return 2;
        }
    }
    // refused sizes
    {
        uint8_t s[32] = {0}, c[128];
        if (eth::make_cache(s, 0, c) || eth::make_cache(s, 63, c) || eth::make_cache(s, 100, c))
            return fail("a cache size that is no positive multiple of 64 was accepted");
    }
    // the reciprocal reduction: cache rows and dataset pages of epochs 0, 1 and 2047, and the edge divisors
    std::vector<uint32_t> rows = {1u, 2u, 16u, 0xFFFFFFFFu};
    for (uint64_t e : {0ull, 1ull, 2047ull}) {
        rows.push_back((uint32_t)(eth::calc_cache_size(e) / 64));
        rows.push_back((uint32_t)(eth::calc_dataset_size(e) / 128));
    }
    for (uint32_t r : rows)
        if (!check_mod(r)) return fail("mod_reduce for rows = " + std::to_string(r));
    std::cout << "ok\n";
    return 0;
}

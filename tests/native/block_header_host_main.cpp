// Stand-alone check of csrc/block_header_host.h (plain C++: built by tests/test_block_header_cpu.py with ASan +
// UBSan): the record layout, the configuration as the kernels take it, and the compaction / gather / scatter of
// the headers whose seal is checked.  Prints "ok".
#include <cstdio>
#include <cstdlib>

#include "../../geth-sharding_amd/csrc/block_header_host.h"

using namespace gsv::bh;

#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); \
            return 1;                                              \
        }                                                          \
    } while (0)

static uint64_t rnd(uint64_t& s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

int main() {
    // layout: the parts tile the work area in order, rows of 8-byte values stay 8-byte aligned for every n
    for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(64), size_t(65), size_t(2048), size_t(262144)}) {
        const RecordOffsets o = record_offsets(n);
        const size_t m = n + 1;
        CHECK(o.hash == 0 && o.parent_hash == 32 * m && o.difficulty == 64 * m && o.time == 96 * m);
        CHECK(o.number == 128 * m && o.gas_limit == 136 * m && o.gas_used == 144 * m && o.flags == 152 * m);
        CHECK(o.end == work_bytes(n) && o.end == REC_BYTES * m && REC_BYTES == 156);
        CHECK(o.number % 8 == 0 && o.gas_limit % 8 == 0 && o.gas_used % 8 == 0 && o.flags % 4 == 0);
    }
    // every record byte is touched exactly once by a writer that follows the offsets
    {
        const size_t n = 37;
        const RecordOffsets o = record_offsets(n);
        std::vector<uint8_t> work(work_bytes(n), 0);
        const size_t start[8] = {o.hash, o.parent_hash, o.difficulty, o.time, o.number, o.gas_limit, o.gas_used, o.flags};
        const size_t width[8] = {32, 32, 32, 32, 8, 8, 8, 4};
        for (int part = 0; part < 8; part++)
            for (size_t i = 0; i <= n; i++)
                for (size_t b = 0; b < width[part]; b++) work.at(start[part] + i * width[part] + b)++;
        for (uint8_t v : work) CHECK(v == 1);
    }
    // the configuration
    {
        gsv_chain_config g;
        std::memset(&g, 0, sizeof g);
        Config c = make_config(g);
        CHECK(c.flags == 0);
        g.homestead_block = 1150000, g.has_homestead = 1;
        g.dao_fork_block = 1920000, g.has_dao_fork = 1, g.dao_fork_support = 1;
        g.eip150_block = 2463000, g.has_eip150 = 1;
        g.byzantium_block = 4370000, g.has_byzantium = 7;  // any non-zero byte is "present"
        for (int k = 0; k < 32; k++) g.eip150_hash[k] = (uint8_t)(k + 1);
        c = make_config(g);
        CHECK(c.flags == (C_HOMESTEAD | C_DAO | C_EIP150 | C_BYZANTIUM | C_DAO_SUPPORT | C_EIP150_HASH));
        CHECK(c.homestead == 1150000 && c.dao == 1920000 && c.eip150 == 2463000 && c.byzantium == 4370000);
        CHECK(c.eip150_hash[0] == 0x04030201u && c.eip150_hash[7] == 0x201F1E1Du);
        std::memset(g.eip150_hash, 0, 32);
        g.eip150_hash[31] = 1;
        CHECK(make_config(g).flags & C_EIP150_HASH);
        g.eip150_hash[31] = 0;
        CHECK(!(make_config(g).flags & C_EIP150_HASH));
        CHECK(sizeof(gsv_chain_config) == 72);
    }
    // compaction, gather, scatter against a plain restatement
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (size_t n : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(64), size_t(65), size_t(257), size_t(2048)}) {
        for (int with_seals = 0; with_seals < 2; with_seals++) {
            std::vector<uint8_t> pre(n), seals(n), rows(n * 32), nonce_rows(n * 8);
            for (size_t i = 0; i < n; i++) {
                pre[i] = rnd(s) % 3 == 0 ? (uint8_t)(20 + rnd(s) % 13) : 0;
                seals[i] = rnd(s) % 4 != 0;
                for (int b = 0; b < 32; b++) rows[i * 32 + b] = (uint8_t)rnd(s);
                for (int b = 0; b < 8; b++) nonce_rows[i * 8 + b] = (uint8_t)rnd(s);
            }
            std::vector<uint32_t> idx;
            compact_sealed(pre.data(), with_seals ? seals.data() : nullptr, n, idx);
            size_t want = 0;
            for (size_t i = 0; i < n; i++) {
                const bool in = pre[i] == 0 && (!with_seals || seals[i]);
                if (in) {
                    CHECK(want < idx.size() && idx[want] == i);  // in input order
                    want++;
                }
            }
            CHECK(want == idx.size());
            std::vector<uint8_t> g32, g8;
            gather_rows(rows.data(), 32, idx, g32);
            gather_rows(nonce_rows.data(), 8, idx, g8);
            CHECK(g32.size() == idx.size() * 32 && g8.size() == idx.size() * 8);
            for (size_t k = 0; k < idx.size(); k++) {
                CHECK(std::memcmp(&g32[k * 32], &rows[(size_t)idx[k] * 32], 32) == 0);
                CHECK(std::memcmp(&g8[k * 8], &nonce_rows[(size_t)idx[k] * 8], 8) == 0);
            }
            std::vector<uint8_t> st(idx.size()), out;
            for (size_t k = 0; k < idx.size(); k++) st[k] = (uint8_t)(16 + rnd(s) % 3);
            scatter_status(st, idx, n, out);
            CHECK(out.size() == n);
            size_t k = 0;
            for (size_t i = 0; i < n; i++) {
                if (k < idx.size() && idx[k] == i) CHECK(out[i] == st[k++]);
                else CHECK(out[i] == 0);
            }
        }
    }
    std::printf("ok\n");
    return 0;
}

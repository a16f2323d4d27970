// Stand-alone check of the staging plans of the host-pointer entry points (csrc/staging.h): builds the
// *Stage declarations the entry points build and checks, for each, that every offset is 256-aligned,
// the buffers are pairwise disjoint, the last one ends at or before the Layout's total, that total is
// exactly the buffers' rounded sizes (so no buffer of the struct is missing from the list here), and
// the per-call temporary shape, which shape_temp places at the total, starts past all of them.
// Absent optional buffers reserve nothing and bind to nullptr.  Prints "ok <plans>" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/staging.h"

using namespace gsv::api;

struct Region { const char* name; size_t off, bytes; bool present; };

static int g_fail = 0, g_plans = 0;
static uint8_t* const kBase = (uint8_t*)(uintptr_t)0x10000;  // never dereferenced

template <typename T>
static Region reg(const char* name, const Buf<T>& b, bool present = true) {
    if (present != (b(kBase) != nullptr)) {
        printf("FAIL %s: present=%d but pointer %p\n", name, (int)present, (void*)b(kBase));
        g_fail++;
    }
    return {name, b.off, b.bytes, present};
}

// `base`: where the plan's first buffer must start (the partition's own block starts at `gathered`)
static void check(const std::string& plan, const Layout& L, const std::vector<Region>& rs, size_t base = 0) {
    g_plans++;
    auto fail = [&](const char* what, const Region& r) {
        printf("FAIL %s: %s (%s off=%zu bytes=%zu total=%zu)\n", plan.c_str(), what, r.name, r.off, r.bytes, L.n);
        g_fail++;
    };
    size_t sum = base, first = ~(size_t)0;
    for (size_t i = 0; i < rs.size(); i++) {
        const Region& a = rs[i];
        if (!a.present) continue;
        if (a.off % 256) fail("offset not 256-aligned", a);
        if (a.off + a.bytes > L.n) fail("ends past the total", a);
        first = a.off < first ? a.off : first;
        sum += al(a.bytes ? a.bytes : 1);
        for (size_t j = i + 1; j < rs.size(); j++) {
            const Region& b = rs[j];
            // zero-length buffers too must not share an address (each holds at least its 256-B slot)
            if (b.present && a.off < b.off + (b.bytes ? b.bytes : 1) && b.off < a.off + (a.bytes ? a.bytes : 1))
                fail("overlaps another buffer", a);
        }
    }
    const size_t shape_off = L.n;  // shape_temp(c, staged, ..): c->arena + staged.n
    if (shape_off % 256) fail("temporary shape offset not aligned", rs[0]);
    if (sum != L.n || (first != ~(size_t)0 && first != base)) fail("total is not the sum of the buffers", rs[0]);
}

int main() {
    const size_t body_len[3] = {4097, 0, 1};  // n = 1 takes the first
    for (size_t n : {(size_t)1, (size_t)3})
        for (bool opt : {false, true}) {
            const std::string tag = " n=" + std::to_string(n) + (opt ? " +opt" : " -opt");
            size_t bytes = 0, pos = 0;  // packed bytes, and with 16-byte aligned starts (stage_offsets)
            for (size_t i = 0; i < n; i++) {
                bytes += body_len[i];
                pos = (pos + body_len[i] + 15) & ~(size_t)15;
            }
            const uint32_t max_txs = 5;
            {
                Layout L;
                KeccakStage p(L, bytes, n);
                check("keccak256_batch" + tag, L, {reg("data", p.data), reg("off", p.off), reg("out", p.out)});
            }
            {
                Layout L;
                EcrecoverStage p(L, n, opt, opt);
                check("ecrecover_batch" + tag, L,
                      {reg("msg", p.msg), reg("sig", p.sig), reg("pub", p.pub, opt), reg("addr", p.addr, opt),
                       reg("st", p.st)});
            }
            for (size_t rec : {(size_t)128, (size_t)96}) {  // ecrecover precompile / bn256Add, bn256ScalarMul
                Layout L;
                RecordStage p(L, n, rec, rec == 128 && !opt ? 32 : 64);
                check("record_batch" + tag, L, {reg("in", p.in), reg("out", p.out), reg("st", p.st)});
            }
            auto sender = [](const SenderStage& s) {
                return std::vector<Region>{reg("h", s.h), reg("r", s.r), reg("s", s.s), reg("v", s.v),
                                           reg("vb", s.vb), reg("a", s.a), reg("st", s.st)};
            };
            {
                Layout L;
                SenderStage p(L, n);
                check("sender_batch" + tag, L, sender(p));
            }
            {
                Layout L;
                TxSenderStage p(L, bytes, n);
                std::vector<Region> rs{reg("pre", p.pre), reg("poff", p.poff)};
                for (const Region& r : sender(p.snd)) rs.push_back(r);
                check("tx_sender_batch" + tag, L, rs);
            }
            {
                Layout L;
                SynthSignStage p(L, n, opt, opt);
                check("synth_sign" + tag, L,
                      {reg("msg", p.msg), reg("sig", p.sig), reg("pub", p.pub, opt), reg("addr", p.addr, opt)});
            }
            for (const char* name : {"chunk_root_batch", "derive_sha_batch", "collation_poc_batch"}) {
                Layout L;
                RootsStage p(L, pos, n);
                check(name + tag, L, {reg("in", p.in), reg("roots", p.roots)});
            }
            {
                Layout L;
                PairingStage p(L, bytes, n);
                check("pairing_check_batch" + tag, L, {reg("in", p.in), reg("verdict", p.verdict)});
            }
            auto notary = [&](const NotaryStage& s) {
                return std::vector<Region>{reg("bodies", s.bodies),          reg("root", s.root),
                                           reg("ntx", s.ntx),                reg("bitmap", s.bitmap),
                                           reg("senders", s.senders, opt),   reg("status", s.status, opt)};
            };
            {
                Layout L;
                NotaryStage p(L, pos, n, max_txs, opt, opt);
                check("notary_validate_shards" + tag, L, notary(p));
            }
            // the partition: n shards on one rank, and 3 shards over 2 ranks seen from either rank
            for (int ranks : {1, 2}) {
                const size_t n_total = ranks == 1 ? n : 3;
                for (int r = 0; r < ranks; r++) {
                    const PartDims d = part_dims(n_total, ranks, r, max_txs);
                    Layout L;
                    PartitionStage p(L, d, n_total, ranks, d.n ? pos : 0, max_txs, opt, opt);
                    std::vector<Region> out{reg("blk", p.blk), reg("all", p.all), reg("oroot", p.oroot),
                                            reg("ontx", p.ontx), reg("obm", p.obm), reg("rst", p.rst)};
                    Layout G;  // what a failing rank reserves: the gathered part alone
                    G.n = p.gathered;
                    check("notary_validate_partition (gathered)" + tag, G, out);
                    std::vector<Region> all = out;
                    for (const Region& q : notary(p.own)) all.push_back(q);
                    check("notary_validate_partition" + tag, L, all);
                    check("notary_validate_partition (own block)" + tag, L, notary(p.own), p.gathered);
                }
            }
            {
                Layout L;
                HeaderStage p(L, n, n * 96 + 7, opt, opt, opt);
                check("collation_header_verify_batch" + tag, L,
                      {reg("sid", p.sid), reg("root", p.root), reg("per", p.per), reg("prop", p.prop),
                       reg("sig", p.sig), reg("nil", p.nil, opt), reg("hash", p.hash, opt),
                       reg("signer", p.signer, opt), reg("st", p.st), reg("scr", p.scr)});
            }
            {
                Layout L;
                BlockMergeStage p(L, n);
                check("ethash_verify_headers_batch (merge)" + tag, L,
                      {reg("pre", p.pre), reg("seal", p.seal), reg("post", p.post), reg("out", p.out)});
                for (const B8* b : {&p.pre, &p.seal, &p.post, &p.out})  // a status byte per header, each way
                    if (b->bytes != n) {
                        printf("FAIL merge stage%s: a buffer of %zu bytes for %zu headers\n", tag.c_str(), b->bytes, n);
                        g_fail++;
                    }
            }
        }
    // the partition with an empty local block (n = 0, n_total = 3, 2 ranks): part_dims leaves a rank
    // without shards only when n_total < ranks, so the block is emptied by hand here, and the real case
    // (1 shard over 2 ranks, rank 0) follows
    {
        PartDims d = part_dims(3, 2, 0, 5);
        d.n = 0;
        Layout L;
        PartitionStage p(L, d, 3, 2, 0, 5, true, true);
        std::vector<Region> rs{reg("blk", p.blk),       reg("all", p.all),           reg("oroot", p.oroot),
                               reg("ontx", p.ontx),     reg("obm", p.obm),           reg("rst", p.rst),
                               reg("bodies", p.own.bodies), reg("root", p.own.root), reg("ntx", p.own.ntx),
                               reg("bitmap", p.own.bitmap), reg("senders", p.own.senders),
                               reg("status", p.own.status)};
        check("notary_validate_partition n=0 of 3, 2 ranks", L, rs);
        const PartDims e = part_dims(1, 2, 0, 5);  // a real empty block: 1 shard over 2 ranks, rank 0
        if (e.n != 0) {
            printf("FAIL part_dims(1, 2, 0): n = %zu\n", e.n);
            g_fail++;
        }
        Layout M;
        PartitionStage q(M, e, 1, 2, 0, 5, false, false);
        check("notary_validate_partition n=0 of 1, 2 ranks", M,
              {reg("blk", q.blk), reg("all", q.all), reg("oroot", q.oroot), reg("ontx", q.ontx), reg("obm", q.obm),
               reg("rst", q.rst), reg("bodies", q.own.bodies), reg("root", q.own.root), reg("ntx", q.own.ntx),
               reg("bitmap", q.own.bitmap), reg("senders", q.own.senders, false),
               reg("status", q.own.status, false)});
    }
    if (g_fail) {
        printf("%d failure(s)\n", g_fail);
        return 1;
    }
    printf("ok %d\n", g_plans);
    return 0;
}

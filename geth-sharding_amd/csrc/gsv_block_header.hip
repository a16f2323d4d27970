// Block headers of the C ABI (gsv_ctx.h): the device forms check their arguments and enqueue launches of
// block_header.hip; the host forms stage a chain segment, run decode + rules, bring Number and the pre-seal status
// back, hand the sealed headers that have passed so far to the ethash host path (grouped by epoch over the
// context's caches, gsv_ethash.hip) and merge the three statuses on the device.
#include "gsv_ctx.h"

using namespace gsv::api;
namespace bh = gsv::bh;

namespace {

constexpr uint64_t MAX_N = 0x7FFFFFFFull;
constexpr uint64_t MAX_NOW = 1ull << 63;  // now + 15 stays in uint64

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// stages items [off[0], off[n]) at the stage's start and their offsets rebased to zero
int stage_items(Staged& s, const BlockHeaderStage& p, const uint8_t* rlp, const uint64_t* off, size_t n) {
    const std::vector<uint64_t> rel = table_rebase(off, n);
    GSVCHK(s.in(p.rlp, rlp + off[0], rel[n]));
    return s.in(p.off, rel.data());
}

int decode_launch(gsv_ctx* c, const uint8_t* d_rlp, const uint64_t* d_off, size_t n, const uint8_t* d_parent,
                  size_t parent_len, uint8_t* d_work, uint8_t* d_hash32, uint8_t* d_hnn32, uint64_t* d_nonce,
                  uint8_t* d_mix32, uint8_t* d_diff32, uint64_t* d_number, uint8_t* d_status, hipStream_t st) {
    KTimer t(c, GSV_K_BLOCK_HEADER, st);
    return hip_err(gsv::launch_block_header(d_rlp, d_off, (uint32_t)n, d_parent, (uint32_t)parent_len, d_work, d_hash32,
                                            d_hnn32, d_nonce, d_mix32, d_diff32, d_number, d_status, st));
}

}  // namespace

extern "C" {

size_t gsv_block_header_work_bytes(size_t n) { return bh::work_bytes(n); }

int gsv_block_header_rules_dev(gsv_ctx* c, const gsv_chain_config* config, const uint8_t* d_rlp, const uint64_t* d_off,
                               size_t n, const uint8_t* d_parent_rlp, size_t parent_len, uint64_t now, uint8_t* d_work,
                               uint8_t* d_hash_no_nonce32, uint64_t* d_nonce, uint8_t* d_mix32, uint8_t* d_difficulty32,
                               uint8_t* d_pre_status, uint8_t* d_post_status, uint8_t* d_hash32, uint64_t* d_number,
                               uint8_t* d_expected_difficulty32, void* stream) {
    if (!c || !config || n > MAX_N || parent_len > MAX_N || now > MAX_NOW) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!d_rlp || !d_off || !aligned(d_off, 8) || (parent_len && !d_parent_rlp) || !d_work || !aligned(d_work, 16) ||
        !d_hash_no_nonce32 || !aligned(d_hash_no_nonce32, 4) || !d_nonce || !aligned(d_nonce, 8) || !d_mix32 ||
        !d_difficulty32 || !d_pre_status || !d_post_status || !aligned(d_number, 8))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    int rc = decode_launch(c, d_rlp, d_off, n, d_parent_rlp, parent_len, d_work, d_hash32, d_hash_no_nonce32, d_nonce,
                           d_mix32, d_difficulty32, d_number, nullptr, st);
    if (rc) return rc;
    KTimer t(c, GSV_K_BLOCK_RULES, st);
    return hip_err(gsv::launch_block_header_rules(d_work, (uint32_t)n, bh::make_config(*config), now, d_pre_status,
                                                  d_post_status, d_expected_difficulty32, st));
}

int gsv_block_header_merge_dev(gsv_ctx* c, const uint8_t* d_pre_status, const uint8_t* d_seal_status,
                               const uint8_t* d_seals, const uint8_t* d_post_status, size_t n, uint8_t* d_status,
                               void* stream) {
    if (!c || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!d_pre_status || !d_post_status || !d_status) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BLOCK_MERGE, st);
    return hip_err(gsv::launch_block_header_merge(d_pre_status, d_seal_status, d_seals, d_post_status, (uint32_t)n,
                                                  d_status, st));
}

int gsv_block_header_hash_batch(gsv_ctx* c, const uint8_t* rlp, const uint64_t* off, size_t n, uint8_t* hash32,
                                uint8_t* hash_no_nonce32, uint8_t* status) {
    if (!c || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!rlp || !off || !status) return GSV_E_INVALID_ARG;
    GSVCHK(table_check(rlp, off, n, kBelow4G));
    Layout L;
    const BlockHeaderStage p(L, off[n] - off[0], n, 0, bh::work_bytes(n), false, false);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(stage_items(s, p, rlp, off, n));
    GSVCHK(decode_launch(c, s(p.rlp), s(p.off), n, nullptr, 0, s(p.work), s(p.hash), s(p.hnn), nullptr, nullptr, nullptr,
                         nullptr, s(p.pre), c->stream));
    if (hash32) GSVCHK(s.out(hash32, p.hash));
    if (hash_no_nonce32) GSVCHK(s.out(hash_no_nonce32, p.hnn));
    GSVCHK(s.out(status, p.pre));
    return s.finish();
}

int gsv_calc_difficulty_batch(gsv_ctx* c, const gsv_chain_config* config, const uint64_t* time,
                              const uint8_t* parent_rlp, const uint64_t* parent_off, size_t n, uint8_t* difficulty32,
                              uint8_t* status) {
    if (!c || !config || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!time || !parent_rlp || !parent_off || !difficulty32 || !status) return GSV_E_INVALID_ARG;
    GSVCHK(table_check(parent_rlp, parent_off, n, kBelow4G));
    Layout L;
    const BlockHeaderStage p(L, parent_off[n] - parent_off[0], n, 0, bh::work_bytes(n), false, true);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(stage_items(s, p, parent_rlp, parent_off, n));
    GSVCHK(s.in(p.time, time));
    GSVCHK(decode_launch(c, s(p.rlp), s(p.off), n, nullptr, 0, s(p.work), nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, c->stream));
    {
        KTimer t(c, GSV_K_BLOCK_RULES, c->stream);
        GSVCHK(hip_err(gsv::launch_calc_difficulty(s(p.work), (uint32_t)n, bh::make_config(*config), s(p.time),
                                                   s(p.want), s(p.pre), c->stream)));
    }
    GSVCHK(s.out(difficulty32, p.want));
    GSVCHK(s.out(status, p.pre));
    return s.finish();
}

int gsv_ethash_verify_headers_batch(gsv_ctx* c, const gsv_chain_config* config, const uint8_t* rlp, const uint64_t* off,
                                    size_t n, const uint8_t* parent_rlp, size_t parent_len, const uint8_t* seals,
                                    uint64_t now, int test_mode, uint8_t* status, uint8_t* hash32,
                                    uint8_t* expected_difficulty32) {
    if (!c || !config || n > MAX_N || parent_len > MAX_N || now > MAX_NOW) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!rlp || !off || !status || (parent_len && !parent_rlp)) return GSV_E_INVALID_ARG;
    GSVCHK(table_check(rlp, off, n, kBelow4G));
    std::vector<uint64_t> number(n), nonce(n);
    std::vector<uint8_t> pre(n), post(n), hnn(n * 32), mix(n * 32), diff(n * 32);
    std::unique_lock<std::mutex> lk(c->mu);
    {
        // 1. decode + rules
        Layout L;
        const BlockHeaderStage p(L, off[n] - off[0], n, parent_len, bh::work_bytes(n), true, false);
        Staged s(c, L, lk);
        if (s.rc) return s.rc;
        GSVCHK(stage_items(s, p, rlp, off, n));
        GSVCHK(s.in(p.parent, parent_rlp, parent_len));
        GSVCHK(gsv_block_header_rules_dev(c, config, s(p.rlp), s(p.off), n, s(p.parent), parent_len, now, s(p.work),
                                          s(p.hnn), s(p.nonce), s(p.mix), s(p.diff), s(p.pre), s(p.post), s(p.hash),
                                          s(p.number), s(p.want), c->stream));
        // 2. what the seal needs, Number and the two statuses come back
        GSVCHK(s.out(number.data(), p.number));
        GSVCHK(s.out(pre.data(), p.pre));
        GSVCHK(s.out(post.data(), p.post));
        GSVCHK(s.out(hnn.data(), p.hnn));
        GSVCHK(s.out(nonce.data(), p.nonce));
        GSVCHK(s.out(mix.data(), p.mix));
        GSVCHK(s.out(diff.data(), p.diff));
        if (hash32) GSVCHK(s.out(hash32, p.hash));
        if (expected_difficulty32) GSVCHK(s.out(expected_difficulty32, p.want));
        GSVCHK(s.finish());
    }
    // 3. - 5. the sealed headers that have passed so far, by epoch over the context's caches, through the light
    // kernel.  The ethash path stages in the arena too: what the merge reads is staged again behind it.
    std::vector<uint32_t> idx;
    bh::compact_sealed(pre.data(), seals, n, idx);
    std::vector<uint8_t> seal_st(n, GSV_ST_OK);
    if (!idx.empty()) {
        const size_t m = idx.size();
        std::vector<uint8_t> h2, m2, d2, st2(m);
        bh::gather_rows(hnn.data(), 32, idx, h2);
        bh::gather_rows(mix.data(), 32, idx, m2);
        bh::gather_rows(diff.data(), 32, idx, d2);
        std::vector<uint64_t> nonce2(m), number2(m);
        for (size_t k = 0; k < m; k++) {
            nonce2[k] = nonce[idx[k]];
            number2[k] = number[idx[k]];
        }
        GSVCHK(ethash_verify_seal_host(c, lk, number2.data(), test_mode != 0, h2.data(), nonce2.data(), m2.data(),
                                       d2.data(), m, st2.data()));
        bh::scatter_status(st2, idx, n, seal_st);
    }
    // 6. merge
    Layout L;
    const BlockMergeStage p(L, n);
    Staged s(c, L, lk);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.pre, pre.data()));
    GSVCHK(s.in(p.seal, seal_st.data()));
    GSVCHK(s.in(p.post, post.data()));
    // the compaction already applied seals[]: every status left in p.seal counts
    GSVCHK(gsv_block_header_merge_dev(c, s(p.pre), s(p.seal), nullptr, s(p.post), n, s(p.out), c->stream));
    GSVCHK(s.out(status, p.out));
    return s.finish();
}

}  // extern "C"

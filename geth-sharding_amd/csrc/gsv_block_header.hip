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

// every item shorter than 2^32 bytes, offsets ascending
int check_offsets(const uint64_t* off, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return GSV_E_INVALID_ARG;
        if (off[i + 1] - off[i] > 0xFFFFFFFFull) return GSV_E_TOO_LARGE;
    }
    return GSV_SUCCESS;
}

// stages items [off[0], off[n]) at the stage's start and their offsets rebased to zero
int stage_items(gsv_ctx* c, const BlockHeaderStage& p, const uint8_t* rlp, const uint64_t* off, size_t n,
                std::vector<uint64_t>& rebased) {
    rebased.resize(n + 1);
    for (size_t i = 0; i <= n; i++) rebased[i] = off[i] - off[0];
    if (rebased[n]) HIPCHK(hipMemcpyAsync(p.rlp(c->arena), rlp + off[0], rebased[n], hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(p.off(c->arena), rebased.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return GSV_SUCCESS;
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
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
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
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_BLOCK_MERGE, st);
    return hip_err(gsv::launch_block_header_merge(d_pre_status, d_seal_status, d_seals, d_post_status, (uint32_t)n,
                                                  d_status, st));
}

int gsv_block_header_hash_batch(gsv_ctx* c, const uint8_t* rlp, const uint64_t* off, size_t n, uint8_t* hash32,
                                uint8_t* hash_no_nonce32, uint8_t* status) {
    if (!c || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!rlp || !off || !status) return GSV_E_INVALID_ARG;
    int rc = check_offsets(off, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const BlockHeaderStage p(L, off[n] - off[0], n, 0, bh::work_bytes(n), false, false);
    rc = arena_reserve(c, L.n);
    if (rc) return rc;
    std::vector<uint64_t> rebased;
    rc = stage_items(c, p, rlp, off, n, rebased);
    if (rc) return rc;
    rc = decode_launch(c, p.rlp(c->arena), p.off(c->arena), n, nullptr, 0, p.work(c->arena), p.hash(c->arena),
                       p.hnn(c->arena), nullptr, nullptr, nullptr, nullptr, p.pre(c->arena), c->stream);
    if (rc) return rc;
    if (hash32) HIPCHK(hipMemcpyAsync(hash32, p.hash(c->arena), n * 32, hipMemcpyDeviceToHost, c->stream));
    if (hash_no_nonce32)
        HIPCHK(hipMemcpyAsync(hash_no_nonce32, p.hnn(c->arena), n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, p.pre(c->arena), n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

int gsv_calc_difficulty_batch(gsv_ctx* c, const gsv_chain_config* config, const uint64_t* time,
                              const uint8_t* parent_rlp, const uint64_t* parent_off, size_t n, uint8_t* difficulty32,
                              uint8_t* status) {
    if (!c || !config || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!time || !parent_rlp || !parent_off || !difficulty32 || !status) return GSV_E_INVALID_ARG;
    int rc = check_offsets(parent_off, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const BlockHeaderStage p(L, parent_off[n] - parent_off[0], n, 0, bh::work_bytes(n), false, true);
    rc = arena_reserve(c, L.n);
    if (rc) return rc;
    std::vector<uint64_t> rebased;
    rc = stage_items(c, p, parent_rlp, parent_off, n, rebased);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(p.time(c->arena), time, n * 8, hipMemcpyHostToDevice, c->stream));
    rc = decode_launch(c, p.rlp(c->arena), p.off(c->arena), n, nullptr, 0, p.work(c->arena), nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, c->stream);
    if (rc) return rc;
    {
        KTimer t(c, GSV_K_BLOCK_RULES, c->stream);
        rc = hip_err(gsv::launch_calc_difficulty(p.work(c->arena), (uint32_t)n, bh::make_config(*config),
                                                 p.time(c->arena), p.want(c->arena), p.pre(c->arena), c->stream));
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(difficulty32, p.want(c->arena), n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, p.pre(c->arena), n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

int gsv_ethash_verify_headers_batch(gsv_ctx* c, const gsv_chain_config* config, const uint8_t* rlp, const uint64_t* off,
                                    size_t n, const uint8_t* parent_rlp, size_t parent_len, const uint8_t* seals,
                                    uint64_t now, int test_mode, uint8_t* status, uint8_t* hash32,
                                    uint8_t* expected_difficulty32) {
    if (!c || !config || n > MAX_N || parent_len > MAX_N || now > MAX_NOW) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!rlp || !off || !status || (parent_len && !parent_rlp)) return GSV_E_INVALID_ARG;
    int rc = check_offsets(off, n);
    if (rc) return rc;
    std::vector<uint64_t> rebased, number(n), nonce(n);
    std::vector<uint8_t> pre(n), post(n), hnn(n * 32), mix(n * 32), diff(n * 32);
    std::unique_lock<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    {
        // 1. decode + rules
        Layout L;
        const BlockHeaderStage p(L, off[n] - off[0], n, parent_len, bh::work_bytes(n), true, false);
        rc = arena_reserve(c, L.n);
        if (rc) return rc;
        uint8_t* A = c->arena;
        rc = stage_items(c, p, rlp, off, n, rebased);
        if (rc) return rc;
        if (parent_len) HIPCHK(hipMemcpyAsync(p.parent(A), parent_rlp, parent_len, hipMemcpyHostToDevice, c->stream));
        rc = gsv_block_header_rules_dev(c, config, p.rlp(A), p.off(A), n, p.parent(A), parent_len, now, p.work(A),
                                        p.hnn(A), p.nonce(A), p.mix(A), p.diff(A), p.pre(A), p.post(A), p.hash(A),
                                        p.number(A), p.want(A), c->stream);
        if (rc) return rc;
        // 2. what the seal needs, Number and the two statuses come back
        HIPCHK(hipMemcpyAsync(number.data(), p.number(A), n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(pre.data(), p.pre(A), n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(post.data(), p.post(A), n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(hnn.data(), p.hnn(A), n * 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(nonce.data(), p.nonce(A), n * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(mix.data(), p.mix(A), n * 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(diff.data(), p.diff(A), n * 32, hipMemcpyDeviceToHost, c->stream));
        if (hash32) HIPCHK(hipMemcpyAsync(hash32, p.hash(A), n * 32, hipMemcpyDeviceToHost, c->stream));
        if (expected_difficulty32)
            HIPCHK(hipMemcpyAsync(expected_difficulty32, p.want(A), n * 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
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
        rc = ethash_verify_seal_host(c, lk, number2.data(), test_mode != 0, h2.data(), nonce2.data(), m2.data(),
                                     d2.data(), m, st2.data());
        if (rc) return rc;
        bh::scatter_status(st2, idx, n, seal_st);
    }
    // 6. merge
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const B8 d_pre = L.buf(n), d_seal = L.buf(n), d_post = L.buf(n), d_out = L.buf(n);
    rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t* A = c->arena;
    HIPCHK(hipMemcpyAsync(d_pre(A), pre.data(), n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_seal(A), seal_st.data(), n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_post(A), post.data(), n, hipMemcpyHostToDevice, c->stream));
    // the compaction already applied seals[]: every status left in d_seal counts
    rc = gsv_block_header_merge_dev(c, d_pre(A), d_seal(A), nullptr, d_post(A), n, d_out(A), c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(status, d_out(A), n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

}  // extern "C"

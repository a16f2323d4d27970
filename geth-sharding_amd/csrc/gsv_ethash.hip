// ethash of the C ABI (gsv_ctx.h): the device forms check their arguments and enqueue launches of ethash.hip
// (one each; the search three nodes); the host forms group a batch by epoch, keep the epochs' verification
// caches on the device (made on the host by ethash_host.h, outside the context's lock) and, for the full and
// seal forms, the epochs' datasets (made on the device from those caches), and run one launch per epoch, the
// sealer one search per round.
#include <map>

#include "ethash_host.h"
#include "gsv_ctx.h"

using namespace gsv::api;
namespace eth = gsv::ethash;

namespace {

constexpr uint64_t MAX_DATASET = 1ull << 38;  // rows <= 2^31: 2 parent + 1 fits 32 bits
constexpr uint64_t MAX_N = 0x7FFFFFFFull;     // two lanes per header in a 32-bit grid

bool cache_ok(const uint8_t* d_cache, uint64_t cache_bytes) {
    return d_cache && ((uintptr_t)d_cache & 15) == 0 && cache_bytes >= eth::HASH_BYTES &&
           cache_bytes % eth::HASH_BYTES == 0 && cache_bytes < MAX_DATASET;
}

bool dataset_ok(uint64_t dataset_bytes) {
    return dataset_bytes >= eth::MIX_BYTES && dataset_bytes % eth::MIX_BYTES == 0 && dataset_bytes <= MAX_DATASET;
}

bool full_dataset_ok(const uint8_t* d_dataset, uint64_t dataset_bytes) {
    return d_dataset && ((uintptr_t)d_dataset & 127) == 0 && dataset_ok(dataset_bytes);
}

bool seed_ok(const uint8_t* d_hash32, const uint64_t* d_nonce) {
    return d_hash32 && d_nonce && ((uintptr_t)d_hash32 & 3) == 0 && ((uintptr_t)d_nonce & 7) == 0;
}

// the first full-size epoch whose dataset no longer fits MAX_DATASET: the host forms refuse it (and every
// later one) before sizing anything
constexpr uint64_t MAX_EPOCH = (MAX_DATASET - eth::DATASET_INIT_BYTES) / eth::DATASET_GROWTH_BYTES;

struct EpochSizes {
    uint64_t cache_bytes, dataset_bytes;
};

EpochSizes epoch_sizes(uint64_t epoch, bool test) {
    if (test) return {eth::TEST_CACHE_BYTES, eth::TEST_DATASET_BYTES};
    return {eth::calc_cache_size(epoch), eth::calc_dataset_size(epoch)};
}

// The device cache of (epoch, test), called with the context's lock held.  On a miss the lock is dropped
// while the host generates the cache (a second for a full-size epoch: ADVICE's second finding, no long
// work under the mutex), then the list is searched again.  Every host form synchronises before it
// releases the lock, so whoever holds it knows that no launch is reading any cached pointer: the
// eviction's hipFree is never under running work.
int epoch_cache(gsv_ctx* c, std::unique_lock<std::mutex>& lk, uint64_t epoch, bool test, const EpochSizes& sz,
                const uint8_t** d_cache) {
    auto find = [&]() {
        for (auto it = c->ethash_caches.begin(); it != c->ethash_caches.end(); ++it)
            if (it->epoch == epoch && it->test == test) {
                c->ethash_caches.splice(c->ethash_caches.begin(), c->ethash_caches, it);  // most recently used
                return true;
            }
        return false;
    };
    if (!find()) {
        lk.unlock();
        std::vector<uint8_t> host(sz.cache_bytes);
        uint8_t seed[32];
        eth::seed_hash(epoch * eth::EPOCH_LENGTH, seed);
        const bool made = eth::make_cache(seed, sz.cache_bytes, host.data());
        lk.lock();
        if (!made) return GSV_E_INVALID_ARG;
        HIPCHK(hipSetDevice(c->device));
        if (!find()) {
            while (c->ethash_caches.size() >= GSV_ETHASH_MAX_CACHES) {
                hipFree(c->ethash_caches.back().d);
                c->ethash_caches.pop_back();
            }
            uint8_t* d = nullptr;
            if (hipMalloc(&d, sz.cache_bytes) != hipSuccess) return GSV_E_NOMEM;
            if (hipMemcpy(d, host.data(), sz.cache_bytes, hipMemcpyHostToDevice) != hipSuccess) {
                hipFree(d);
                return GSV_E_HIP;
            }
            c->ethash_caches.push_front({epoch, test, d, sz.cache_bytes});
        }
    }
    *d_cache = c->ethash_caches.front().d;
    return GSV_SUCCESS;
}

// The device dataset of (epoch, test), called with the context's lock held and nothing of this context's
// running (every host form synchronises before it releases the lock).  On a miss: the epoch's cache (which
// may drop and retake the lock), then the new dataset's memory BEFORE anything is evicted, so a failed
// allocation leaves the list as it was; then the least recently used go, and k_ethash_items fills the new one
// on the context stream, which is waited for.
int epoch_dataset(gsv_ctx* c, std::unique_lock<std::mutex>& lk, uint64_t epoch, bool test, const EpochSizes& sz,
                  const uint8_t** d_dataset) {
    auto find = [&]() {
        for (auto it = c->ethash_datasets.begin(); it != c->ethash_datasets.end(); ++it)
            if (it->epoch == epoch && it->test == test) {
                c->ethash_datasets.splice(c->ethash_datasets.begin(), c->ethash_datasets, it);
                return true;
            }
        return false;
    };
    if (!find()) {
        const uint8_t* d_cache = nullptr;
        int rc = epoch_cache(c, lk, epoch, test, sz, &d_cache);
        if (rc) return rc;
        if (!find()) {  // the lock may have been dropped for the cache: another call may have made it
            HIPCHK(hipSetDevice(c->device));
            uint8_t* d = nullptr;
            if (hipMalloc(&d, sz.dataset_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return GSV_E_NOMEM;
            }
            const uint64_t items = sz.dataset_bytes / eth::HASH_BYTES;
            for (uint64_t first = 0; first < items && rc == GSV_SUCCESS;) {
                const uint64_t count = std::min<uint64_t>(items - first, 1ull << 31);
                rc = gsv_ethash_dataset_items_dev(c, d_cache, sz.cache_bytes, first, count, d + first * eth::HASH_BYTES,
                                                  c->stream);
                first += count;
            }
            if (rc == GSV_SUCCESS && hipStreamSynchronize(c->stream) != hipSuccess) rc = GSV_E_HIP;
            if (rc) {
                hipFree(d);
                return rc;
            }
            while (c->ethash_datasets.size() >= GSV_ETHASH_MAX_DATASETS) {
                hipFree(c->ethash_datasets.back().d);
                c->ethash_datasets.pop_back();
            }
            c->ethash_datasets.push_front({epoch, test, d, sz.dataset_bytes});
        }
    }
    *d_dataset = c->ethash_datasets.front().d;
    return GSV_SUCCESS;
}

// groups item indices by epoch; GSV_E_TOO_LARGE for an epoch whose dataset passes MAX_DATASET
int group_by_epoch(const uint64_t* number, size_t n, bool test, std::map<uint64_t, std::vector<uint32_t>>& groups) {
    for (size_t i = 0; i < n; i++) {
        const uint64_t epoch = number[i] / eth::EPOCH_LENGTH;
        if (!test && epoch >= MAX_EPOCH) return GSV_E_TOO_LARGE;
        groups[epoch].push_back((uint32_t)i);
    }
    return GSV_SUCCESS;
}

// light / full: a / b are the outputs (mix digest, result); verify: the inputs (mix digest, difficulty).  full
// reads the epoch's dataset instead of its cache.
// With the context's lock held in `lk`.
int host_batch_locked(gsv_ctx* c, std::unique_lock<std::mutex>& lk, const uint64_t* number, bool test,
                      const uint8_t* hash32, const uint64_t* nonce, size_t n, bool verify, bool full,
                      const uint8_t* a_in, const uint8_t* b_in, uint8_t* a_out, uint8_t* b_out, uint8_t* status) {
    if (!c || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!number || !hash32 || !nonce) return GSV_E_INVALID_ARG;
    if (verify ? (!a_in || !b_in || !status) : (!a_out || !b_out)) return GSV_E_INVALID_ARG;
    std::map<uint64_t, std::vector<uint32_t>> groups;
    int grc = group_by_epoch(number, n, test, groups);
    if (grc) return grc;
    std::vector<uint8_t> h, a, b, st;
    std::vector<uint64_t> nn;
    for (const auto& g : groups) {
        const std::vector<uint32_t>& items = g.second;
        const size_t m = items.size();
        const EpochSizes sz = epoch_sizes(g.first, test);
        const uint8_t *d_cache = nullptr, *d_dataset = nullptr;
        int rc = full ? epoch_dataset(c, lk, g.first, test, sz, &d_dataset)
                      : epoch_cache(c, lk, g.first, test, sz, &d_cache);
        if (rc) return rc;
        h.resize(m * 32);
        nn.resize(m);
        a.resize(m * 32);
        b.resize(m * 32);
        st.resize(m);
        for (size_t k = 0; k < m; k++) {
            const size_t i = items[k];
            memcpy(&h[k * 32], hash32 + i * 32, 32);
            nn[k] = nonce[i];
            if (verify) {
                memcpy(&a[k * 32], a_in + i * 32, 32);
                memcpy(&b[k * 32], b_in + i * 32, 32);
            }
        }
        Layout L;
        const EthashStage p(L, m, verify);
        Staged s(c, L, lk);
        if (s.rc) return s.rc;
        GSVCHK(s.in(p.hash, h.data()));
        GSVCHK(s.in(p.nonce, nn.data()));
        if (verify) {
            GSVCHK(s.in(p.a, a.data()));
            GSVCHK(s.in(p.b, b.data()));
            GSVCHK(gsv_ethash_verify_seal_batch_dev(c, d_cache, sz.cache_bytes, sz.dataset_bytes, s(p.hash), s(p.nonce),
                                                    s(p.a), s(p.b), m, s(p.st), c->stream));
            GSVCHK(s.out(st.data(), p.st));
        } else {
            GSVCHK(full ? gsv_ethash_full_batch_dev(c, d_dataset, sz.dataset_bytes, s(p.hash), s(p.nonce), m, s(p.a),
                                                    s(p.b), c->stream)
                        : gsv_ethash_light_batch_dev(c, d_cache, sz.cache_bytes, sz.dataset_bytes, s(p.hash), s(p.nonce),
                                                     m, s(p.a), s(p.b), c->stream));
            GSVCHK(s.out(a.data(), p.a));
            GSVCHK(s.out(b.data(), p.b));
        }
        GSVCHK(s.finish());
        for (size_t k = 0; k < m; k++) {
            const size_t i = items[k];
            if (verify) {
                status[i] = st[k];
            } else {
                memcpy(a_out + i * 32, &a[k * 32], 32);
                memcpy(b_out + i * 32, &b[k * 32], 32);
            }
        }
    }
    return GSV_SUCCESS;
}

int host_batch(gsv_ctx* c, const uint64_t* number, bool test, const uint8_t* hash32, const uint64_t* nonce, size_t n,
               bool verify, bool full, const uint8_t* a_in, const uint8_t* b_in, uint8_t* a_out, uint8_t* b_out,
               uint8_t* status) {
    if (!c) return GSV_E_INVALID_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    return host_batch_locked(c, lk, number, test, hash32, nonce, n, verify, full, a_in, b_in, a_out, b_out, status);
}

}  // namespace

namespace gsv {
namespace api {

int ethash_verify_seal_host(gsv_ctx* c, std::unique_lock<std::mutex>& lk, const uint64_t* number, bool test,
                            const uint8_t* hash32, const uint64_t* nonce, const uint8_t* mix32,
                            const uint8_t* difficulty32, size_t n, uint8_t* status) {
    return host_batch_locked(c, lk, number, test, hash32, nonce, n, true, false, mix32, difficulty32, nullptr, nullptr,
                             status);
}

}  // namespace api
}  // namespace gsv

extern "C" {

int gsv_ethash_dataset_items_dev(gsv_ctx* c, const uint8_t* d_cache, uint64_t cache_bytes, uint64_t first,
                                 uint64_t count, uint8_t* d_out64, void* stream) {
    if (!c || !cache_ok(d_cache, cache_bytes) || first > (1ull << 32) || count > (1ull << 32) - first)
        return GSV_E_INVALID_ARG;
    if (count == 0) return GSV_SUCCESS;
    if (!d_out64 || ((uintptr_t)d_out64 & 15) || count > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ETHASH_ITEMS, st);
    return hip_err(gsv::launch_ethash_items(d_cache, cache_bytes, (uint32_t)first, (uint32_t)count, d_out64, st));
}

int gsv_ethash_light_batch_dev(gsv_ctx* c, const uint8_t* d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                               const uint8_t* d_hash32, const uint64_t* d_nonce, size_t n, uint8_t* d_mix32,
                               uint8_t* d_result32, void* stream) {
    if (!c || !cache_ok(d_cache, cache_bytes) || !dataset_ok(dataset_bytes) || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!seed_ok(d_hash32, d_nonce) || !d_mix32 || !d_result32) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ETHASH_LIGHT, st);
    return hip_err(gsv::launch_ethash_light(d_cache, cache_bytes, dataset_bytes, d_hash32, d_nonce, (uint32_t)n,
                                            d_mix32, d_result32, st));
}

int gsv_ethash_verify_seal_batch_dev(gsv_ctx* c, const uint8_t* d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                                     const uint8_t* d_hash32, const uint64_t* d_nonce, const uint8_t* d_mix32,
                                     const uint8_t* d_difficulty32, size_t n, uint8_t* d_status, void* stream) {
    if (!c || !cache_ok(d_cache, cache_bytes) || !dataset_ok(dataset_bytes) || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!seed_ok(d_hash32, d_nonce) || !d_mix32 || !d_difficulty32 || !d_status) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ETHASH_LIGHT, st);
    return hip_err(gsv::launch_ethash_verify(d_cache, cache_bytes, dataset_bytes, d_hash32, d_nonce, d_mix32,
                                             d_difficulty32, (uint32_t)n, d_status, st));
}

int gsv_ethash_light_batch(gsv_ctx* c, const uint64_t* number, int test_mode, const uint8_t* hash32,
                           const uint64_t* nonce, size_t n, uint8_t* mix32_out, uint8_t* result32_out) {
    return host_batch(c, number, test_mode != 0, hash32, nonce, n, false, false, nullptr, nullptr, mix32_out,
                      result32_out, nullptr);
}

int gsv_ethash_verify_seal_batch(gsv_ctx* c, const uint64_t* number, const uint8_t* hash32, const uint64_t* nonce,
                                 const uint8_t* mix32, const uint8_t* difficulty32, size_t n, int test_mode,
                                 uint8_t* status) {
    return host_batch(c, number, test_mode != 0, hash32, nonce, n, true, false, mix32, difficulty32, nullptr, nullptr,
                      status);
}

int gsv_ethash_full_batch_dev(gsv_ctx* c, const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                              const uint64_t* d_nonce, size_t n, uint8_t* d_mix32, uint8_t* d_result32, void* stream) {
    if (!c || !full_dataset_ok(d_dataset, dataset_bytes) || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!seed_ok(d_hash32, d_nonce) || !d_mix32 || !d_result32) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ETHASH_FULL, st);
    return hip_err(gsv::launch_ethash_full(d_dataset, dataset_bytes, d_hash32, d_nonce, (uint32_t)n, d_mix32,
                                           d_result32, st));
}

int gsv_ethash_verify_seal_full_batch_dev(gsv_ctx* c, const uint8_t* d_dataset, uint64_t dataset_bytes,
                                          const uint8_t* d_hash32, const uint64_t* d_nonce, const uint8_t* d_mix32,
                                          const uint8_t* d_difficulty32, size_t n, uint8_t* d_status, void* stream) {
    if (!c || !full_dataset_ok(d_dataset, dataset_bytes) || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!seed_ok(d_hash32, d_nonce) || !d_mix32 || !d_difficulty32 || !d_status) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ETHASH_FULL, st);
    return hip_err(gsv::launch_ethash_verify_full(d_dataset, dataset_bytes, d_hash32, d_nonce, d_mix32,
                                                  d_difficulty32, (uint32_t)n, d_status, st));
}

int gsv_ethash_search_dev(gsv_ctx* c, const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                          const uint8_t* d_difficulty32, const uint64_t* d_start, size_t n, uint64_t span,
                          uint32_t* d_offset, uint64_t* d_nonce_out, uint8_t* d_mix32, uint8_t* d_result32,
                          uint8_t* d_found, void* stream) {
    if (!c || !full_dataset_ok(d_dataset, dataset_bytes) || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (span == 0 || span > 0xFFFFFFFFull || (uint64_t)n * ((span + 255) / 256) > MAX_N) return GSV_E_INVALID_ARG;
    if (!seed_ok(d_hash32, d_start) || !d_difficulty32 || !d_offset || ((uintptr_t)d_offset & 3) || !d_nonce_out ||
        ((uintptr_t)d_nonce_out & 7) || !d_mix32 || !d_result32 || !d_found)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    // A 32-bit fill, not hipMemsetAsync(.., 0xFF, 4 n).  An observation, seen in one test run and not traced
    // to its cause: with the byte form captured into a graph and d_offset at 4 mod 16, the three words in front
    // of the first 16-byte boundary read zero after the replay, so those headers "won" at offset 0; the same
    // call outside a capture filled them.  tests/test_gpu_ethash_full.py test_dev_form_contract keeps d_offset
    // at 4 mod 16 and passes with this form.
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d_offset, (int)0xFFFFFFFFu, n, st));
    {
        KTimer t(c, GSV_K_ETHASH_SEARCH, st);
        int rc = hip_err(gsv::launch_ethash_search(d_dataset, dataset_bytes, d_hash32, d_difficulty32, d_start,
                                                   (uint32_t)n, (uint32_t)span, d_offset, st));
        if (rc) return rc;
    }
    KTimer t(c, GSV_K_ETHASH_FINISH, st);
    return hip_err(gsv::launch_ethash_finish(d_dataset, dataset_bytes, d_hash32, d_start, d_offset, (uint32_t)n,
                                             d_nonce_out, d_mix32, d_result32, d_found, st));
}

int gsv_ethash_full_batch(gsv_ctx* c, const uint64_t* number, int test_mode, const uint8_t* hash32,
                          const uint64_t* nonce, size_t n, uint8_t* mix32_out, uint8_t* result32_out) {
    return host_batch(c, number, test_mode != 0, hash32, nonce, n, false, true, nullptr, nullptr, mix32_out,
                      result32_out, nullptr);
}

int gsv_ethash_seal_batch(gsv_ctx* c, const uint64_t* number, int test_mode, const uint8_t* hash32,
                          const uint8_t* difficulty32, const uint64_t* start_nonce, size_t n, uint64_t max_attempts,
                          uint64_t* nonce_out, uint8_t* mix32_out, uint8_t* status) {
    if (!c || n > MAX_N) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!number || !hash32 || !difficulty32 || !start_nonce || !nonce_out || !mix32_out || !status)
        return GSV_E_INVALID_ARG;
    const bool test = test_mode != 0;
    std::map<uint64_t, std::vector<uint32_t>> groups;
    int rc = group_by_epoch(number, n, test, groups);
    if (rc) return rc;
    memset(nonce_out, 0, n * sizeof(uint64_t));
    memset(mix32_out, 0, n * 32);
    static const uint8_t zero32[32] = {0};
    std::vector<uint8_t> h, d, mix, found;
    std::vector<uint64_t> start, won;
    std::unique_lock<std::mutex> lk(c->mu);
    for (const auto& g : groups) {
        // the headers still searching, with the nonce each tries next; all have been tried `tried` times
        std::vector<uint32_t> items;
        std::vector<uint64_t> next;
        for (uint32_t i : g.second) {
            if (memcmp(difficulty32 + (size_t)i * 32, zero32, 32) == 0) {
                status[i] = GSV_ST_INVALID_DIFFICULTY;
                continue;
            }
            status[i] = GSV_ST_NONCE_NOT_FOUND;
            items.push_back(i);
            next.push_back(start_nonce[i]);
        }
        if (items.empty() || max_attempts == 0) continue;
        const EpochSizes sz = epoch_sizes(g.first, test);
        const uint8_t* d_dataset = nullptr;
        rc = epoch_dataset(c, lk, g.first, test, sz, &d_dataset);
        if (rc) return rc;
        for (uint64_t tried = 0; tried < max_attempts && !items.empty();) {
            const eth::SealRound round = eth::seal_round(items.size(), max_attempts - tried);
            std::vector<uint32_t> keep_items;
            std::vector<uint64_t> keep_next;
            for (size_t at = 0; at < items.size(); at += round.headers) {
                const size_t m = std::min<size_t>(round.headers, items.size() - at);
                h.resize(m * 32);
                d.resize(m * 32);
                mix.resize(m * 32);
                found.resize(m);
                start.resize(m);
                won.resize(m);
                for (size_t k = 0; k < m; k++) {
                    memcpy(&h[k * 32], hash32 + (size_t)items[at + k] * 32, 32);
                    memcpy(&d[k * 32], difficulty32 + (size_t)items[at + k] * 32, 32);
                    start[k] = next[at + k];
                }
                Layout L;
                const EthashSealStage p(L, m);
                Staged s(c, L, lk);
                if (s.rc) return s.rc;
                GSVCHK(s.in(p.hash, h.data()));
                GSVCHK(s.in(p.diff, d.data()));
                GSVCHK(s.in(p.start, start.data()));
                GSVCHK(gsv_ethash_search_dev(c, d_dataset, sz.dataset_bytes, s(p.hash), s(p.diff), s(p.start), m,
                                             round.span, s(p.offset), s(p.nonce), s(p.mix), s(p.result), s(p.found),
                                             c->stream));
                GSVCHK(s.out(won.data(), p.nonce));
                GSVCHK(s.out(mix.data(), p.mix));
                GSVCHK(s.out(found.data(), p.found));
                GSVCHK(s.finish());
                for (size_t k = 0; k < m; k++) {
                    const uint32_t i = items[at + k];
                    if (found[k]) {
                        status[i] = GSV_ST_OK;
                        nonce_out[i] = won[k];
                        memcpy(mix32_out + (size_t)i * 32, &mix[k * 32], 32);
                    } else {
                        keep_items.push_back(i);
                        keep_next.push_back(next[at + k] + round.span);  // mod 2^64
                    }
                }
            }
            items.swap(keep_items);
            next.swap(keep_next);
            tried += round.span;
        }
    }
    return GSV_SUCCESS;
}

int gsv_ctx_ethash_datasets(gsv_ctx* c, size_t* count) {
    if (!c || !count) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    *count = c->ethash_datasets.size();
    return GSV_SUCCESS;
}

int gsv_ctx_ethash_caches(gsv_ctx* c, size_t* count) {
    if (!c || !count) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    *count = c->ethash_caches.size();
    return GSV_SUCCESS;
}

}  // extern "C"

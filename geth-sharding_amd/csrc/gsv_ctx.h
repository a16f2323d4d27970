// Internals of the C ABI of libgsv.so (include/gsv.h), shared by its translation units:
//   gsv_ctx.hip      context, streams, kernel timing, staging arena, the cache of prepared shapes
//   gsv_batch.hip    stateless batches: Keccak, ecrecover and its precompile, bn256 add / mul, senders
//   gsv_hash.hip     SHA-256, RIPEMD-160, and the host form the three hashes share (hash_host)
//   gsv_ecies.hip    ecies.Encrypt / Decrypt: the launch chains around the ladder
//   gsv_txsign.hip   types.SignTx: the launch chain around the signature kernel
//   gsv_modexp.hip   the modexp precompile: host grouping by modulus width, one launch per class
//   gsv_ethash.hip   ethash: dataset items, hashimotoLight / Full, VerifySeal, Seal; the epochs' caches and datasets
//   gsv_block_header.hip  types.Header hashes, CalcDifficulty, Ethash.VerifyHeaders: the launch chain around the seal
//   gsv_receipt.hip  bloom9, CreateBloom and the receipt half of ValidateState: the launch chain around DeriveSha
//   gsv_bloombits.hip  the bloombits generator, the bitset codec, the matcher and bloomFilter
//   gsv_clique.hip   clique's voting snapshot and fold behind opaque handles: host only, it uses nothing of this header
//   gsv_trie.hip     chunk root, DeriveSha, Proof of Custody, collation headers
//   gsv_pairing.hip  BN254 pairing check
//   gsv_notary.hip   notary validation, shard partition + RCCL all-gather
//   gsv_proposer.hip blob codec (Serialize / Deserialize), createCollation
// and two headers free of HIP: staging.h (the staged buffers of every host form, declared once) and
// offset_table.h (the rule for a caller's offset table, its rebased copy, fixed records).
//
// Host-pointer entry points stage through a grow-only device arena on the context's stream and are
// synchronous: check the arguments (offset_table.h), declare the *Stage (staging.h), open a Staged (below),
// copy in, call the _dev form, copy out, finish.  *_dev entry points take HBM-resident buffers and the caller's stream and only
// enqueue: they never allocate and never synchronize, so they can be captured into a HIP graph.
// Everything a *_dev call derives from its host-side arguments (trie plans per body length, device
// copies of offset tables, pairing lane tables, its workspace) lives in a PREPARED SHAPE built by the
// matching gsv_*_prepare call (which may allocate and synchronize) and cached per context, keyed by
// exactly those host-side arguments.  A *_dev call whose shape was not prepared returns
// GSV_E_NOT_PREPARED without touching the device.  With a pipeline depth D > 1
// (gsv_ctx_set_pipeline_depth) a shape holds D instances of its device memory, so calls of the same
// shape on up to D streams run concurrently (a notary validating consecutive collation batches keeps
// the latency-bound top of one batch's trie under the next batch's leaf level).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <vector>

#include "chunk_root.h"
#include "gsv_internal.h"
#include "offset_table.h"
#include "staging.h"

struct ncclComm;  // rccl.h (gsv_notary.hip)

namespace gsv {
namespace api {

enum ShapeKind : uint64_t {
    SK_CHUNK = 1, SK_PAIRING = 2, SK_NOTARY = 3, SK_DERIVE = 4, SK_POC = 5, SK_HEADER = 6, SK_PARTITION = 7,
    SK_BLOB_SER = 8, SK_BLOB_DESER = 9, SK_PROPOSER = 10
};

// scatter run: roots of group positions [from, from + count) go to output indices [dst, dst + count)
struct Run { uint32_t dst, from, count; };

// one launch of the trie-plan kernels over the bodies (or lists) of one length
struct TrieGroup {
    std::shared_ptr<gsv::TriePlan> plan;
    uint32_t count = 0;
    size_t koff = 0;      // chunk: first entry in the body-offset table
    bool direct = false;  // chunk: roots written in place (one group holding bodies 0..n-1 in order)
    size_t o_roots = 0, o_scr = 0, o_base = 0;
    std::vector<Run> runs;
};

// chunk roots of a set of bodies (d_bodies[start[i] .. end[i]))
struct ChunkLaunch {
    std::vector<TrieGroup> groups;
    std::vector<uint32_t> empty;  // zero-length bodies -> emptyRoot
    size_t o_off = 0, o_empty = 0;
};

struct Shape {
    uint64_t kind = 0;
    std::vector<uint64_t> key;
    uint8_t* mem = nullptr;
    size_t bytes = 0;   // one instance
    int ninst = 1;      // instances of the device memory (pipeline depth at prepare time)
    int cur = 0;        // instance of the run in progress (set by shape_run under the context's smu)
    int rr = 0;         // next instance to recycle when every instance was last used on another stream
    bool owned = true;  // false: carved from the host-path arena
    std::vector<hipEvent_t> ev;     // per instance: recorded after its last (non-captured) use
    std::vector<hipStream_t> last;  // per instance: stream of that use
    // pipelined instances: per instance, recorded where its last run's bulk kernels ended
    // (GSV_HOOK_TAIL); the next run on another instance starts its bulk kernels after that point
    std::vector<hipEvent_t> bulk_ev;
    std::vector<char> bulk_rec;
    int prev = -1;  // instance of the previous run
    std::vector<std::pair<size_t, std::vector<uint8_t>>> uploads;  // host tables, copied at prepare
    // per instance, the side stream and fork/join events of a shape that runs two launch chains at
    // once (the notary's chunk roots beside its transactions), created at prepare
    std::vector<hipStream_t> side;
    std::vector<hipEvent_t> efork, ejoin;
    bool side_borrowed = false;  // host-path shape: the context's side stream and events, not its own
    int* side_queues = nullptr;  // prepared shape: the context's count of live side queues (own streams)
    ChunkLaunch chunk;  // SK_CHUNK, SK_NOTARY, SK_POC, SK_PARTITION

    // what each kind adds (a kind reads its own part only; SK_PARTITION also uses `notary`, for the
    // rank's own block)
    struct Pairing {
        size_t np = 0, nl = 0, nchecks = 0;
        int layout = 0;  // GSV_BN_LAYOUT_* flags
        size_t o_src = 0, o_pidx = 0, o_lfirst = 0, o_clane = 0, o_cbad = 0, o_pstat = 0, o_lines = 0, o_lstat = 0,
               o_fv = 0, o_fws = 0;
        uint32_t maxl = 1;  // the most Miller lanes of any check
        int deep = 0;       // pairing layout class of the depth it was prepared at (bn_depth_class)
    } pairing;
    struct Notary {
        uint32_t max_txs = 0, sfx_len = 0;
        int signer_kind = 0;
        size_t o_cid = 0, o_noff = 0, o_nlen = 0, o_cnt = 0, o_blobs = 0;
    } notary;
    struct Derive {
        std::vector<TrieGroup> groups;
        std::vector<uint32_t> empty;
        size_t o_voff = 0, o_lmsg = 0, o_leafrefs = 0, o_empty = 0;
        uint64_t vend = 0;  // end of the batch's value bytes (absolute offset into the caller's vals)
    } derive;
    struct Poc {
        size_t o_io = 0, o_oo = 0, o_salt = 0, o_out = 0;
        uint64_t max = 0;
        uint32_t salt_len = 0;
    } poc;
    struct Header {
        size_t o_scr = 0;
    } header;
    struct Part {
        size_t n = 0, total = 0;
        int ranks = 1, rank = 0;
        size_t o_lroot = 0, o_lntx = 0, o_lbm = 0, o_block = 0, o_all = 0;
    } part;
    struct BlobSer {  // SK_BLOB_SER, SK_PROPOSER: the serialize plan (gsv_proposer.hip)
        size_t o_ents = 0, o_cidx = 0, o_over = 0;
        uint64_t nchunks = 0, begin = 0, end = 0, first_blob = 0;
        bool any_over = false;
    } ser;
    struct BlobDeser {  // SK_BLOB_DESER
        size_t o_off = 0, o_len = 0, o_doff = 0, o_recs = 0;
        uint64_t begin = 0, end = 0, max_region = 0;
    } deser;

    Shape() = default;
    Shape(const Shape&) = delete;
    Shape& operator=(const Shape&) = delete;
    // the shape's own side streams (hardware queues) and events; a borrowed set stays the context's
    void release_side() {
        if (!side_borrowed) {
            for (hipStream_t q : side)
                if (q) {
                    hipStreamSynchronize(q);
                    hipStreamDestroy(q);
                    if (side_queues) --*side_queues;
                }
            for (hipEvent_t e : efork)
                if (e) hipEventDestroy(e);
            for (hipEvent_t e : ejoin)
                if (e) hipEventDestroy(e);
        }
        side.clear();
        efork.clear();
        ejoin.clear();
    }
    ~Shape() {
        release_side();
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        for (hipEvent_t e : bulk_ev)
            if (e) hipEventDestroy(e);
        if (owned && mem) hipFree(mem);
    }
    template <typename T>
    void stage(size_t off, const T* p, size_t count) {
        if (!count) return;
        const uint8_t* b = (const uint8_t*)p;
        uploads.emplace_back(off, std::vector<uint8_t>(b, b + count * sizeof(T)));
    }
    template <typename T>
    T* at(size_t off) const { return (T*)(mem + (size_t)cur * bytes + off); }
};

}  // namespace api
}  // namespace gsv

struct gsv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint4* gtab = nullptr;
    // grow-only staging arena for the host-pointer entry points
    uint8_t* arena = nullptr;
    size_t arena_cap = 0;
    std::mutex mu;
    // kernel timing
    int timing = 0;
    struct Pending { int kid; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    double total_ms[GSV_K_RIDGE] = {0};
    long launches[GSV_K_RIDGE] = {0};
    std::mutex tmu;
    std::vector<hipEvent_t> open_ev;  // timer events opened by launch hooks
    hipStream_t cur_stream = nullptr;  // stream of the shape run in progress (launch hooks)
    bool cur_capture = false;          // that run is being captured into a graph: no timer events
    gsv::api::Shape* cur_shape = nullptr;  // the shape of that run (GSV_HOOK_TAIL marks)
    // trie plans per body length, prepared shapes (most recently used first)
    gsv::PlanCache plans;
    std::list<std::unique_ptr<gsv::api::Shape>> shapes;
    size_t shape_bytes = 0;
    std::mutex smu;  // shapes, cur_stream / cur_capture
    // RCCL communicator of the shard partition (gsv_comm_init), nullptr = single rank
    ncclComm* comm = nullptr;
    int nranks = 1, rank = 0;
    // completion of the last all-gather issued on `comm`: the next one, possibly on another stream (a
    // pipelined partition call), waits for it, so collectives on the communicator never overlap
    hipEvent_t coll_ev = nullptr;
    bool coll_rec = false;
    std::mutex cmu;  // the collective: coll_ev / coll_rec and the ncclAllGather issue order
    // the host paths' side stream and fork/join events (lent to their per-call shapes)
    hipStream_t hside = nullptr;
    hipEvent_t hfork = nullptr, hjoin = nullptr;
    // live side streams of the prepared shapes (each shape owns its own, on hardware queues of their
    // own, own_queue_stream: HIP's four shared in-order queues would order a side chain after unrelated
    // work; the notary pipeline two deep measured 11,734 vs 11,419 shards/s, profiles/r05/ab/notary_sweep_*)
    int side_queues = 0;
    // streams made by gsv_stream_create, destroyed by gsv_stream_destroy or with the context
    std::vector<hipStream_t> user_streams;
    std::mutex qmu;
    int pipeline_depth = 1;  // instances per prepared shape (gsv_ctx_set_pipeline_depth)
    // the ethash host forms' verification caches on the device, most recently used first, at most
    // GSV_ETHASH_MAX_CACHES (gsv_ethash.hip); guarded by mu
    struct EthashCache {
        uint64_t epoch;
        bool test;
        uint8_t* d;
        uint64_t bytes;
    };
    std::list<EthashCache> ethash_caches;
    // the epochs' datasets, generated on the device for the full and seal host forms: the same record, at
    // most GSV_ETHASH_MAX_DATASETS, the same rule for freeing one
    std::list<EthashCache> ethash_datasets;
};

namespace gsv {
namespace api {

inline int hip_err(hipError_t e) { return e == hipSuccess ? GSV_SUCCESS : GSV_E_HIP; }

#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t _e = (x);                       \
        if (_e != hipSuccess) return GSV_E_HIP;    \
    } while (0)

#define GSVCHK(x)               \
    do {                        \
        int _rc = (x);          \
        if (_rc) return _rc;    \
    } while (0)

// the stream of a *_dev call: the caller's, or the context's
inline hipStream_t stream_of(gsv_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }
// the kernels index a batch with 32 bits
inline bool batch_too_long(size_t n) { return n > 0xFFFFFFFFull; }

int arena_reserve(gsv_ctx* c, size_t bytes);

// One host form's turn at the staging arena, opened after the argument checks: holds the context's lock (its
// own, or one the caller holds already and may drop and retake between two turns), sets the device and
// reserves what the stage declared.  `rc` is the outcome of that; the entry point returns it when nonzero.
// Then in() and out() copy between host memory and a staged buffer on the context's stream, and finish()
// waits for the stream.  A copy is as long as the buffer was declared (Buf::bytes) or a stated shorter
// length; one that would pass the buffer's end fails with GSV_E_INVALID_ARG and enqueues nothing.  An absent
// buffer (an optional output not asked for) and a copy of no bytes are skipped.
// A pointer into the arena is bound by s(buf), and only after the call's LAST reservation: arena_reserve may
// move the arena, and a form with a per-call shape reserves in shape_temp (kWithShape leaves it to that).
// secret() names the region that holds key material from the next copy on: [key.off, key.off + key.bytes), or
// [0, end) of a stage that puts every secret first.  It is overwritten on the context's stream, and the stream
// waited for, on every way out that follows (GSVCHK's and HIPCHK's early returns included); finish() is the
// success path's last step and reports the outcome of both calls.
struct Staged {
    enum Reserve { kNow, kWithShape };
    gsv_ctx* c;
    std::unique_lock<std::mutex> own;  // empty when the caller's lock was adopted
    int rc;
    size_t wipe_off = 0, wipe_bytes = 0;

    Staged(gsv_ctx* c_, const Layout& L, Reserve r = kNow) : c(c_), own(c_->mu), rc(open(L, r)) {}
    Staged(gsv_ctx* c_, const Layout& L, std::unique_lock<std::mutex>& held) : c(c_), rc(open(L, kNow)) {
        if (!held.owns_lock()) rc = GSV_E_INVALID_ARG;
    }
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
    ~Staged() {
        if (wipe_bytes) finish();
    }

    template <typename T>
    T* operator()(const Buf<T>& b) const { return b(c->arena); }
    template <typename T>
    int in(const Buf<T>& b, const void* src) { return in(b, src, b.bytes); }
    template <typename T>
    int in(const Buf<T>& b, const void* src, size_t bytes) {
        if (b.off == kAbsent || !bytes) return GSV_SUCCESS;
        if (bytes > b.bytes) return GSV_E_INVALID_ARG;
        return hip_err(hipMemcpyAsync(c->arena + b.off, src, bytes, hipMemcpyHostToDevice, c->stream));
    }
    template <typename T>
    int out(void* dst, const Buf<T>& b) { return out(dst, b, b.bytes); }
    template <typename T>
    int out(void* dst, const Buf<T>& b, size_t bytes) {
        if (b.off == kAbsent || !bytes) return GSV_SUCCESS;
        if (bytes > b.bytes) return GSV_E_INVALID_ARG;
        return hip_err(hipMemcpyAsync(dst, c->arena + b.off, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    void secret(const B8& key) { wipe_off = key.off, wipe_bytes = key.bytes; }
    void secret(size_t end) { wipe_off = 0, wipe_bytes = end; }
    int finish() {
        hipError_t a = wipe_bytes ? hipMemsetAsync(c->arena + wipe_off, 0, wipe_bytes, c->stream) : hipSuccess;
        wipe_bytes = 0;
        hipError_t b = hipStreamSynchronize(c->stream);
        return hip_err(a != hipSuccess ? a : b);
    }

private:
    int open(const Layout& L, Reserve r) {
        HIPCHK(hipSetDevice(c->device));
        return r == kNow ? arena_reserve(c, L.n) : GSV_SUCCESS;
    }
};

inline bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) return false;
    return cs != hipStreamCaptureStatusNone;
}

// ---- gsv_ctx.hip
hipEvent_t take_event(gsv_ctx* c);
// timer hooks for multi-launch paths (chunk-root levels, pairing stages)
void hook_begin(void* ctx, int kid);
void hook_end(void* ctx, int kid);
int device_cus(int device);
int shape_materialize(Shape& s, size_t bytes, uint8_t* carve = nullptr, int ninst = 1);
Shape* shape_find(gsv_ctx* c, uint64_t kind, const std::vector<uint64_t>& key);
void shape_insert(gsv_ctx* c, std::unique_ptr<Shape> s);
int shape_pick(Shape& s, hipStream_t st, bool cap);
int shape_side_init(gsv_ctx* c, Shape& s);
int shape_side_borrow(gsv_ctx* c, Shape& s);
// ---- gsv_hash.hip: the host form of gsv_keccak256_batch, gsv_sha256_batch and gsv_ripemd160_batch
typedef hipError_t (*hash_launch)(const uint8_t*, const uint64_t*, uint32_t, uint8_t*, hipStream_t);
int hash_host(gsv_ctx* c, int kid, hash_launch launch, const uint8_t* data, const uint64_t* off, size_t n,
              uint8_t* out32);
// ---- gsv_trie.hip: chunk roots of bodies grouped by length, shared with the notary
int chunk_prepare(gsv_ctx* c, Shape& s, ChunkLaunch& cl, Layout& L, const uint64_t* start, const uint64_t* end,
                  size_t n, uint64_t max_len);
int chunk_run(gsv_ctx* c, const Shape& s, const ChunkLaunch& cl, const uint8_t* d_bodies, uint8_t* d_roots,
              hipStream_t st);
uint64_t stage_offsets(const uint64_t* off, size_t n, std::vector<uint64_t>& st, std::vector<uint64_t>& en);
int stage_bodies(gsv_ctx* c, uint8_t* d_b, const uint8_t* bodies, const uint64_t* off, size_t n,
                 const std::vector<uint64_t>& st, const std::vector<uint64_t>& en);
// generic DeriveSha as a shape, for a host form that runs it between launches of its own (gsv_receipt.hip): item k
// = d_vals[voff[k] .. voff[k+1]), list i = items [list_off[i], list_off[i+1])
int derive_prepare(gsv_ctx* c, Shape& s, const uint64_t* voff, const uint64_t* list_off, size_t n, Layout& L);
int derive_launch(gsv_ctx* c, const Shape& s, const uint8_t* d_vals, uint8_t* d_roots, hipStream_t st);
// ---- gsv_ethash.hip: VerifySeal's checks over host arrays grouped by epoch (gsv_ethash_verify_seal_batch), for a
// caller that holds the context's lock `lk` (it may be dropped and retaken while a cache is generated).  Uses the
// arena and synchronises.
int ethash_verify_seal_host(gsv_ctx* c, std::unique_lock<std::mutex>& lk, const uint64_t* number, bool test,
                            const uint8_t* hash32, const uint64_t* nonce, const uint8_t* mix32,
                            const uint8_t* difficulty32, size_t n, uint8_t* status);
// ---- gsv_pairing.hip
int bn_depth_class(int depth);
// ---- gsv_notary.hip
void comm_destroy(gsv_ctx* c);

// Brackets one launch with events on the launching stream when timing is on (never inside a capture).
struct KTimer {
    gsv_ctx* c;
    int kid;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    KTimer(gsv_ctx* c_, int kid_, hipStream_t st_) : c(c_), kid(kid_), st(st_) {
        if (c->timing && !capturing(st)) {
            std::lock_guard<std::mutex> g(c->tmu);
            a = take_event(c);
            b = take_event(c);
            hipEventRecord(a, st);
        }
    }
    ~KTimer() {
        if (a) {
            hipEventRecord(b, st);
            std::lock_guard<std::mutex> g(c->tmu);
            c->pending.push_back({kid, a, b});
        }
    }
};

// Runs a shape's launches on `st`.  Users of one shape on different streams are ordered on the GPU
// (the workspace is the shape's); inside a stream capture no event is touched, and the caller orders
// graph replays against other uses of the same shape.
template <typename F>
int shape_run(gsv_ctx* c, Shape& s, hipStream_t st, F&& body) {
    bool cap = capturing(st);
    int k = shape_pick(s, st, cap);
    s.cur = k;
    if (!cap && s.ev[k] && s.last[k] && s.last[k] != st) HIPCHK(hipStreamWaitEvent(st, s.ev[k], 0));
    if (!cap && !s.bulk_ev.empty()) {
        // staggered pipeline: this run's bulk kernels follow the previous run's (on the other
        // instance), so they overlap that run's latency-bound tail rather than its bulk kernels
        if (s.prev >= 0 && s.prev != k && s.bulk_rec[s.prev]) HIPCHK(hipStreamWaitEvent(st, s.bulk_ev[s.prev], 0));
        s.bulk_rec[k] = 0;
        s.prev = k;
    }
    c->cur_stream = st;
    c->cur_capture = cap;
    c->cur_shape = &s;
    int rc = body();
    c->cur_shape = nullptr;
    s.cur = 0;
    if (rc) return rc;
    if (!cap && s.ev[k]) {
        HIPCHK(hipEventRecord(s.ev[k], st));
        s.last[k] = st;
    }
    return GSV_SUCCESS;
}

inline void key_push_bytes(std::vector<uint64_t>& key, const uint8_t* p, size_t n) {
    key.push_back(n);
    for (size_t i = 0; i < n; i += 8) {
        uint64_t w = 0;
        memcpy(&w, p + i, std::min<size_t>(8, n - i));
        key.push_back(w);
    }
}

// Prepare-or-find: returns the cached shape for (kind, key), building it with `build` on a miss.
template <typename B>
int shape_get(gsv_ctx* c, uint64_t kind, std::vector<uint64_t>&& key, B&& build, Shape** out) {
    Shape* s = shape_find(c, kind, key);
    // a pairing shape's layout depends on the depth class it was prepared at (three or more batches in
    // flight pick the work-efficient layout, pairing_shape): a prepare at the other class rebuilds it
    const bool reclass = s && kind == SK_PAIRING && s->pairing.deep != bn_depth_class(c->pipeline_depth);
    if (s && (s->ninst < c->pipeline_depth || reclass)) {
        // prepared before the depth was raised (or at the other depth class): build a new one, and
        // RETIRE the old one instead of freeing it (it is never found again but keeps its memory until
        // LRU eviction, which drains its queued work first), so a graph captured from it stays valid.
        // Its side streams go now (a captured graph holds no streams): the new shape needs the queues.
        s->kind |= 1ull << 63;
        bool cap = false;  // a capture still open on a side stream keeps it until eviction
        for (hipStream_t q : s->side) cap = cap || (q && capturing(q));
        if (!cap) s->release_side();
        s = nullptr;
    }
    if (!s) {
        auto ns = std::make_unique<Shape>();
        Layout L;
        int rc = build(*ns, L);
        if (rc) return rc;
        rc = shape_materialize(*ns, L.n, nullptr, c->pipeline_depth);
        if (rc) return rc;
        ns->kind = kind;
        ns->key = std::move(key);
        s = ns.get();
        shape_insert(c, std::move(ns));
    }
    *out = s;
    return GSV_SUCCESS;
}

// Host-path shape: built per call in the arena right after the staged buffers declared in `staged`
// (its offset is their total), run, synchronized.
template <typename B>
int shape_temp(gsv_ctx* c, const Layout& staged, B&& build, Shape& s) {
    Layout L;
    int rc = build(s, L);
    if (rc) return rc;
    rc = arena_reserve(c, staged.n + L.n);
    if (rc) return rc;
    return shape_materialize(s, L.n, c->arena + staged.n);
}

}  // namespace api
}  // namespace gsv

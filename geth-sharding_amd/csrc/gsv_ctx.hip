// The context of the C ABI (gsv_ctx.h): create / destroy, streams, kernel timing and launch hooks, the
// staging arena, and the per-context cache of prepared shapes with their side streams.
#include "gsv_ctx.h"

using namespace gsv::api;

namespace {

constexpr size_t kMaxShapes = 32;
// side streams on hardware queues of their own, over all of a context's prepared shapes: the hardware
// scheduler time-slices queues beyond what it maps at once (r05: ~40 leaked queues ran an 8,192-check
// pairing pipeline at 8.6 instead of 3.8 ms, profiles/r05/ab/pairing_depth_dedicated_leaked_queues.txt);
// a shape prepared past the bound runs its chains one after the other on the caller's stream.
// GSV_MAX_SIDE_STREAMS (0..8) lowers the bound: 0 = no side streams, every notary step runs its chunk
// roots after its transactions on one stream (the leg-only profile pass: tools/profile_round.sh, so no
// dispatch of a traced step overlaps another)
constexpr int kMaxSideQueues = 8;
int max_side_queues() {
    static const int v = [] {
        const char* e = getenv("GSV_MAX_SIDE_STREAMS");
        return e ? std::min(std::max(atoi(e), 0), kMaxSideQueues) : kMaxSideQueues;
    }();
    return v;
}
constexpr size_t kMaxShapeBytes = (size_t)32 << 30;  // of the 288 GB of HBM

void drain_timing(gsv_ctx* c) {
    std::lock_guard<std::mutex> g(c->tmu);
    for (auto& p : c->pending) {
        hipEventSynchronize(p.b);
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->total_ms[p.kid] += ms;
            c->launches[p.kid] += 1;
        }
        c->free_events.push_back(p.a);
        c->free_events.push_back(p.b);
    }
    c->pending.clear();
}

size_t shape_total_bytes(const Shape& s) { return s.bytes * (size_t)s.ninst; }

void shape_drain(Shape& s) {
    for (hipEvent_t e : s.ev)
        if (e) hipEventSynchronize(e);
}

}  // namespace

namespace gsv {
namespace api {

hipEvent_t take_event(gsv_ctx* c) {
    if (!c->free_events.empty()) {
        hipEvent_t e = c->free_events.back();
        c->free_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

void hook_begin(void* p, int kid) {
    gsv_ctx* c = (gsv_ctx*)p;
    if (kid == gsv::GSV_HOOK_TAIL) {  // the run's bulk kernels are enqueued: mark the point for the next run
        Shape* s = c->cur_shape;
        if (s && !c->cur_capture && !s->bulk_ev.empty()) {
            hipEventRecord(s->bulk_ev[s->cur], c->cur_stream);
            s->bulk_rec[s->cur] = 1;
        }
        return;
    }
    if (!c->timing || c->cur_capture) return;
    std::lock_guard<std::mutex> g(c->tmu);
    hipEvent_t a = take_event(c);
    hipEventRecord(a, c->cur_stream);
    c->open_ev.push_back(a);
}
void hook_end(void* p, int kid) {
    gsv_ctx* c = (gsv_ctx*)p;
    if (!c->timing || c->cur_capture) return;
    std::lock_guard<std::mutex> g(c->tmu);
    hipEvent_t a = c->open_ev.back();
    c->open_ev.pop_back();
    hipEvent_t b = take_event(c);
    hipEventRecord(b, c->cur_stream);
    c->pending.push_back({kid, a, b});
}

int arena_reserve(gsv_ctx* c, size_t bytes) {
    if (bytes <= c->arena_cap) return GSV_SUCCESS;
    size_t cap = c->arena_cap ? c->arena_cap : (size_t)64 << 20;
    while (cap < bytes) cap *= 2;
    if (c->arena) {
        hipStreamSynchronize(c->stream);
        hipFree(c->arena);
        c->arena = nullptr;
        c->arena_cap = 0;
    }
    if (hipMalloc(&c->arena, cap) != hipSuccess) return GSV_E_NOMEM;
    c->arena_cap = cap;
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ prepared shapes
// allocates `ninst` instances (or, for a host-path shape, carves one) of the shape's memory and
// uploads its host tables into each
int shape_materialize(Shape& s, size_t bytes, uint8_t* carve, int ninst) {
    bytes = al(bytes ? bytes : 1);
    s.bytes = bytes;
    s.ninst = carve ? 1 : std::max(ninst, 1);
    if (carve) {
        s.mem = carve;
        s.owned = false;
    } else if (hipMalloc(&s.mem, bytes * s.ninst) != hipSuccess) {
        s.mem = nullptr;
        return GSV_E_NOMEM;
    }
    for (int k = 0; k < s.ninst; k++)
        for (auto& u : s.uploads)
            HIPCHK(hipMemcpy(s.mem + (size_t)k * bytes + u.first, u.second.data(), u.second.size(), hipMemcpyHostToDevice));
    s.uploads.clear();
    s.uploads.shrink_to_fit();
    s.ev.assign(s.ninst, nullptr);
    s.last.assign(s.ninst, nullptr);
    if (s.owned)
        for (auto& e : s.ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s.bulk_ev.assign(s.ninst > 1 ? s.ninst : 0, nullptr);
    s.bulk_rec.assign(s.bulk_ev.size(), 0);
    for (auto& e : s.bulk_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return GSV_SUCCESS;
}

Shape* shape_find(gsv_ctx* c, uint64_t kind, const std::vector<uint64_t>& key) {
    for (auto it = c->shapes.begin(); it != c->shapes.end(); ++it) {
        Shape* s = it->get();
        if (s->kind == kind && s->key == key) {
            if (it != c->shapes.begin()) c->shapes.splice(c->shapes.begin(), c->shapes, it);
            return s;
        }
    }
    return nullptr;
}

// inserts a materialized shape; drops least-recently-used shapes beyond the bounds (after their
// queued work has drained — a graph captured from a dropped shape must not be replayed)
void shape_insert(gsv_ctx* c, std::unique_ptr<Shape> s) {
    c->shape_bytes += shape_total_bytes(*s);
    c->shapes.push_front(std::move(s));
    while (c->shapes.size() > 1 && (c->shapes.size() > kMaxShapes || c->shape_bytes > kMaxShapeBytes)) {
        Shape* v = c->shapes.back().get();
        shape_drain(*v);
        c->shape_bytes -= shape_total_bytes(*v);
        c->shapes.pop_back();
    }
}

// The instance a run on `st` uses: the one last used on `st` (the stream orders it), else one never
// used, else the next in turn, ordered after its previous use.  Inside a capture: the instance last
// used on `st`, else instance 0 (the caller orders graph replays against other uses of the shape).
int shape_pick(Shape& s, hipStream_t st, bool cap) {
    for (int k = 0; k < s.ninst; k++)
        if (s.last[k] == st) return k;
    if (cap) return 0;
    for (int k = 0; k < s.ninst; k++)
        if (!s.last[k]) return k;
    int k = s.rr;
    s.rr = (s.rr + 1) % s.ninst;
    return k;
}

int device_cus(int device) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 256;
    return cus;
}

// A stream on an HSA queue of its own: HIP multiplexes ordinary streams over GPU_MAX_HW_QUEUES (4) shared
// in-order queues, but backs a CU-masked stream (here: every CU) by a dedicated queue.  It is ordered with
// the legacy NULL stream like a hipStreamDefault stream.
static int own_queue_stream(int device, hipStream_t* q) {
    const int cus = device_cus(device);
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int i = 0; i < cus; i++) mask[i / 32] |= 1u << (i % 32);
    HIPCHK(hipExtStreamCreateWithCUMask(q, (uint32_t)mask.size(), mask.data()));
    return GSV_SUCCESS;
}

// a side stream and fork/join events per instance (at prepare), for shapes that run two independent
// launch chains at once: the notary's chunk roots beside its transactions.  The streams are
// the SHAPE's own, on hardware queues of their own (a context-wide pool let an uncaptured call
// of one shape enqueue onto a side stream another shape's capture had joined); they live until the shape
// is evicted or retired.  Past kMaxSideQueues live side queues the shape being prepared takes them from
// the least recently used shapes that hold some (those then run their chains one after the other until
// they are prepared again: r06, a sweep over shard counts had left a 13-shard shape holding six queues
// and the next 25-shard shape ran serially, 2.74 instead of 2.15 ms per step).  When that is not enough
// (a capture still open on every candidate's side stream), or HIP refuses a stream or event, the shape
// gets no side streams and runs its chains one after the other on the caller's stream: the results are
// the same and the prepare succeeds (gsv.h).
int shape_side_init(gsv_ctx* c, Shape& s) {
    if (!s.side.empty()) return GSV_SUCCESS;
    const int cap = max_side_queues();
    if (s.ninst > cap) return GSV_SUCCESS;  // serial chains
    for (auto it = c->shapes.rbegin(); it != c->shapes.rend() && c->side_queues + s.ninst > cap; ++it) {
        Shape* v = it->get();
        if (v == &s || v->side.empty() || v->side_borrowed) continue;
        bool open = false;  // a graph being captured through v's side streams keeps them
        for (hipStream_t q : v->side) open = open || (q && capturing(q));
        if (!open) v->release_side();
    }
    if (c->side_queues + s.ninst > cap) return GSV_SUCCESS;  // serial chains
    s.side.assign(s.ninst, nullptr);
    s.efork.assign(s.ninst, nullptr);
    s.ejoin.assign(s.ninst, nullptr);
    s.side_queues = &c->side_queues;
    bool ok = true;
    for (int k = 0; k < s.ninst && ok; k++) {
        ok = own_queue_stream(c->device, &s.side[k]) == GSV_SUCCESS;
        if (ok) c->side_queues++;
        else s.side[k] = nullptr;
        ok = ok && hipEventCreateWithFlags(&s.efork[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&s.ejoin[k], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) s.release_side();  // no partial set
    return GSV_SUCCESS;
}
// a host-path (per-call) shape borrows the context's side stream and events instead of creating its own
int shape_side_borrow(gsv_ctx* c, Shape& s) {
    if (!s.side.empty()) return GSV_SUCCESS;
    if (!c->hside) {
        HIPCHK(hipStreamCreateWithFlags(&c->hside, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->hfork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->hjoin, hipEventDisableTiming));
    }
    s.side.assign(1, c->hside);
    s.efork.assign(1, c->hfork);
    s.ejoin.assign(1, c->hjoin);
    s.side_borrowed = true;
    return GSV_SUCCESS;
}

}  // namespace api
}  // namespace gsv

extern "C" {

int gsv_abi_version(void) { return GSV_ABI_VERSION; }

int gsv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* gsv_error_string(int err) {
    switch (err) {
        case GSV_SUCCESS: return "success";
        case GSV_E_INVALID_ARG: return "invalid argument";
        case GSV_E_HIP: return "HIP runtime error";
        case GSV_E_NOMEM: return "out of device memory";
        case GSV_E_NO_DEVICE: return "no HIP device";
        case GSV_E_TOO_LARGE: return "input exceeds the reference size limit";
        case GSV_E_RCCL: return "RCCL error";
        case GSV_E_NOT_PREPARED: return "batch shape not prepared (call the matching gsv_*_prepare first)";
        default: return "unknown error";
    }
}

int gsv_ctx_create(int device, gsv_ctx** out) {
    if (!out) return GSV_E_INVALID_ARG;
    *out = nullptr;
    int n = gsv_device_count();
    if (n <= 0) return GSV_E_NO_DEVICE;
    if (device < 0 || device >= n) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(device));
    gsv_ctx* c = new gsv_ctx();
    c->device = device;
    // a BLOCKING stream: a *_dev call made with stream = NULL is ordered with the legacy default
    // (NULL) stream of the process both ways — a caller's prior fills and copies there (e.g. PyTorch's
    // default stream) complete before it, and later default-stream work sees its results
    if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) {
        delete c;
        return GSV_E_HIP;
    }
    if (hipMalloc(&c->gtab, gsv::GTAB_BYTES) != hipSuccess) {
        hipStreamDestroy(c->stream);
        delete c;
        return GSV_E_NOMEM;
    }
    hipError_t e = gsv::launch_gtable_init(c->gtab, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        hipFree(c->gtab);
        hipStreamDestroy(c->stream);
        delete c;
        return GSV_E_HIP;
    }
    *out = c;
    return GSV_SUCCESS;
}

void gsv_ctx_destroy(gsv_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();  // every stream's work on the context's shapes has drained
    drain_timing(c);
    for (auto e : c->free_events) hipEventDestroy(e);
    c->shapes.clear();
    {
        std::lock_guard<std::mutex> g(c->qmu);
        for (hipStream_t q : c->user_streams) hipStreamDestroy(q);
        c->user_streams.clear();
    }
    comm_destroy(c);
    if (c->coll_ev) hipEventDestroy(c->coll_ev);
    if (c->hfork) hipEventDestroy(c->hfork);
    if (c->hjoin) hipEventDestroy(c->hjoin);
    if (c->hside) hipStreamDestroy(c->hside);
    for (auto& e : c->ethash_caches) hipFree(e.d);
    for (auto& e : c->ethash_datasets) hipFree(e.d);
    if (c->arena) hipFree(c->arena);
    if (c->gtab) hipFree(c->gtab);
    hipStreamDestroy(c->stream);
    delete c;
}

int gsv_ctx_set_timing(gsv_ctx* c, int enable) {
    if (!c) return GSV_E_INVALID_ARG;
    c->timing = enable ? 1 : 0;
    return GSV_SUCCESS;
}

// A pipeline's streams on queues of their own (gsv.h): r05 measured 8,192-check pairing batches three
// deep at 6.0 or 3.75 ms per batch by which of torch's pool streams the caller took (two of the three on
// one HSA queue in the kernel trace), 3.75 on every set of CU-masked streams
// (profiles/r05/ab/stream_sets_*).
// The context owns them: at most GSV_MAX_STREAMS live at once (more queues oversubscribe the hardware
// scheduler), and gsv_ctx_destroy destroys the ones the caller did not, before the runtime's own teardown.
int gsv_stream_create(gsv_ctx* c, void** stream_out) {
    if (!c || !stream_out) return GSV_E_INVALID_ARG;
    *stream_out = nullptr;
    std::lock_guard<std::mutex> g(c->qmu);
    if (c->user_streams.size() >= GSV_MAX_STREAMS) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t q = nullptr;
    int rc = own_queue_stream(c->device, &q);
    if (rc) return rc;
    c->user_streams.push_back(q);
    *stream_out = (void*)q;
    return GSV_SUCCESS;
}

int gsv_stream_destroy(gsv_ctx* c, void* stream) {
    if (!c || !stream) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->qmu);
    auto it = std::find(c->user_streams.begin(), c->user_streams.end(), (hipStream_t)stream);
    if (it == c->user_streams.end()) return GSV_E_INVALID_ARG;  // not this context's (or already destroyed)
    c->user_streams.erase(it);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamDestroy((hipStream_t)stream));
    return GSV_SUCCESS;
}

int gsv_ctx_stream_count(gsv_ctx* c, int* user_streams, int* side_streams) {
    if (!c) return GSV_E_INVALID_ARG;
    {
        std::lock_guard<std::mutex> g(c->qmu);
        if (user_streams) *user_streams = (int)c->user_streams.size();
    }
    std::lock_guard<std::mutex> g(c->smu);
    if (side_streams) *side_streams = c->side_queues;
    return GSV_SUCCESS;
}

int gsv_ctx_set_pipeline_depth(gsv_ctx* c, int depth) {
    if (!c || depth < 1 || depth > GSV_MAX_PIPELINE_DEPTH) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->smu);
    c->pipeline_depth = depth;
    return GSV_SUCCESS;
}

int gsv_ctx_kernel_time(gsv_ctx* c, int kid, double* total_ms, long* launches) {
    if (!c || kid < 0 || kid >= GSV_K_RIDGE) return GSV_E_INVALID_ARG;
    drain_timing(c);
    if (total_ms) *total_ms = c->total_ms[kid];
    if (launches) *launches = c->launches[kid];
    return GSV_SUCCESS;
}

int gsv_ctx_reset_timing(gsv_ctx* c) {
    if (!c) return GSV_E_INVALID_ARG;
    drain_timing(c);
    for (int i = 0; i < GSV_K_RIDGE; i++) {
        c->total_ms[i] = 0;
        c->launches[i] = 0;
    }
    return GSV_SUCCESS;
}

int gsv_ctx_prepared_shapes(gsv_ctx* c, size_t* count, size_t* device_bytes) {
    if (!c) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->smu);
    if (count) *count = c->shapes.size();
    if (device_bytes) *device_bytes = c->shape_bytes;
    return GSV_SUCCESS;
}

}  // extern "C"

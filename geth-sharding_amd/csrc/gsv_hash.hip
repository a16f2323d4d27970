// The Merkle-Damgard hashes of the C ABI (gsv_ctx.h): SHA-256 and RIPEMD-160 over batches of
// variable-length messages, the sha256hash and ripemd160hash precompiles (core/vm/contracts.go:104-133).
// The conventions are gsv_keccak256_batch's (gsv_batch.hip), whose staging layout the host forms share.
#include <vector>

#include "gsv_ctx.h"

using namespace gsv::api;

namespace {

typedef hipError_t (*md_launch)(const uint8_t*, const uint64_t*, uint32_t, uint8_t*, hipStream_t);

int md_batch_dev(gsv_ctx* c, int kid, md_launch launch, const uint8_t* d_data, const uint64_t* d_off, size_t n,
                 uint8_t* d_out32, void* stream) {
    if (!c || (n && (!d_off || !d_out32)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, kid, st);
    return hip_err(launch(d_data, d_off, (uint32_t)n, d_out32, st));
}

int md_batch(gsv_ctx* c, int kid, md_launch launch, const uint8_t* data, const uint64_t* off, size_t n,
             uint8_t* out32) {
    if (!c || (n && (!off || !out32)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    for (size_t i = 0; i < n; i++)  // the kernels trust off[i] <= off[i+1]
        if (off[i + 1] < off[i]) return GSV_E_INVALID_ARG;
    if (off[n] > off[0] && !data) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    size_t bytes = off[n] - off[0];
    Layout L;
    const KeccakStage p(L, bytes, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t* d_data = p.data(c->arena);
    uint64_t* d_off = p.off(c->arena);
    uint8_t* d_out = p.out(c->arena);
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
    if (bytes) HIPCHK(hipMemcpyAsync(d_data, data + off[0], bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    rc = md_batch_dev(c, kid, launch, d_data, d_off, n, d_out, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out32, d_out, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

}  // namespace

extern "C" {

int gsv_sha256_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n, uint8_t* d_out32,
                         void* stream) {
    return md_batch_dev(c, GSV_K_SHA256, gsv::launch_sha256, d_data, d_off, n, d_out32, stream);
}

int gsv_sha256_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n, uint8_t* out32) {
    return md_batch(c, GSV_K_SHA256, gsv::launch_sha256, data, off, n, out32);
}

int gsv_ripemd160_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n, uint8_t* d_out32,
                            void* stream) {
    return md_batch_dev(c, GSV_K_RIPEMD160, gsv::launch_ripemd160, d_data, d_off, n, d_out32, stream);
}

int gsv_ripemd160_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n, uint8_t* out32) {
    return md_batch(c, GSV_K_RIPEMD160, gsv::launch_ripemd160, data, off, n, out32);
}

}  // extern "C"

// The Merkle-Damgard hashes of the C ABI (gsv_ctx.h): SHA-256 and RIPEMD-160 over batches of
// variable-length messages, the sha256hash and ripemd160hash precompiles (core/vm/contracts.go:104-133).
// The host forms of these two and of gsv_keccak256_batch (gsv_batch.hip) are one routine, hash_host: a table of
// any item length (offset_table.h), the bytes and the rebased table staged in a KeccakStage, one launch.
#include <vector>

#include "gsv_ctx.h"

using namespace gsv::api;

namespace {

int md_batch_dev(gsv_ctx* c, int kid, hash_launch launch, const uint8_t* d_data, const uint64_t* d_off, size_t n,
                 uint8_t* d_out32, void* stream) {
    if (!c || (n && (!d_off || !d_out32)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, kid, st);
    return hip_err(launch(d_data, d_off, (uint32_t)n, d_out32, st));
}

}  // namespace

namespace gsv {
namespace api {

int hash_host(gsv_ctx* c, int kid, hash_launch launch, const uint8_t* data, const uint64_t* off, size_t n,
              uint8_t* out32) {
    if (!c || (n && (!off || !out32)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(data, off, n));  // the kernels trust off[i] <= off[i+1]
    const size_t bytes = off[n] - off[0];
    const std::vector<uint64_t> rel = table_rebase(off, n);
    Layout L;
    const KeccakStage p(L, bytes, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.data, data + off[0], bytes));
    GSVCHK(s.in(p.off, rel.data()));
    {
        KTimer t(c, kid, c->stream);
        HIPCHK(launch(s(p.data), s(p.off), (uint32_t)n, s(p.out), c->stream));
    }
    GSVCHK(s.out(out32, p.out));
    return s.finish();
}

}  // namespace api
}  // namespace gsv

extern "C" {

int gsv_sha256_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n, uint8_t* d_out32,
                         void* stream) {
    return md_batch_dev(c, GSV_K_SHA256, gsv::launch_sha256, d_data, d_off, n, d_out32, stream);
}

int gsv_sha256_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n, uint8_t* out32) {
    return hash_host(c, GSV_K_SHA256, gsv::launch_sha256, data, off, n, out32);
}

int gsv_ripemd160_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n, uint8_t* d_out32,
                            void* stream) {
    return md_batch_dev(c, GSV_K_RIPEMD160, gsv::launch_ripemd160, d_data, d_off, n, d_out32, stream);
}

int gsv_ripemd160_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n, uint8_t* out32) {
    return hash_host(c, GSV_K_RIPEMD160, gsv::launch_ripemd160, data, off, n, out32);
}

}  // extern "C"

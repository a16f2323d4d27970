// Stateless batches of the C ABI (gsv_ctx.h): Keccak-256, ecrecover and its precompile, ECDSA
// verification and public-key parsing, crypto.Sign and public-key derivation, ScalarMult and ECDH,
// bn256Add / bn256ScalarMul, recoverPlain over decoded fields,
// the synthetic signer, types.Sender over tx RLP.
#include <thread>

#include "gsv_ctx.h"
#include "pubkey_pack.h"
#include "tx_host.h"

using namespace gsv::api;

extern "C" {

// ------------------------------------------------------------------ Keccak-256
int gsv_keccak256_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n,
                            uint8_t* d_out32, void* stream) {
    if (!c || (n && (!d_off || !d_out32)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_KECCAK, st);
    return hip_err(gsv::launch_keccak256(d_data, d_off, (uint32_t)n, d_out32, st));
}

int gsv_keccak256_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n,
                        uint8_t* out32) {
    if (!c || (n && (!off || !out32)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    for (size_t i = 0; i < n; i++)  // the kernel trusts off[i] <= off[i+1]
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
    rc = gsv_keccak256_batch_dev(c, d_data, d_off, n, d_out, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out32, d_out, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ ecrecover
int gsv_ecrecover_batch_dev(gsv_ctx* c, const uint8_t* d_msg32, const uint8_t* d_sig65, size_t n,
                            uint8_t* d_pub65, uint8_t* d_addr20, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_msg32 || !d_sig65 || !d_status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecrecover(d_msg32, d_sig65, (uint32_t)n, c->gtab, d_pub65, d_addr20,
                                         d_status, st));
}

int gsv_ecrecover_batch(gsv_ctx* c, const uint8_t* msg32, const uint8_t* sig65, size_t n,
                        uint8_t* pub65_out, uint8_t* addr20_out, uint8_t* status) {
    if (!c || (n && (!msg32 || !sig65 || !status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const EcrecoverStage p(L, n, pub65_out != nullptr, addr20_out != nullptr);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t* d_msg = p.msg(c->arena);
    uint8_t* d_sig = p.sig(c->arena);
    uint8_t* d_pub = p.pub(c->arena);  // nullptr when not asked for
    uint8_t* d_addr = p.addr(c->arena);
    uint8_t* d_st = p.st(c->arena);
    HIPCHK(hipMemcpyAsync(d_msg, msg32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_sig, sig65, n * 65, hipMemcpyHostToDevice, c->stream));
    rc = gsv_ecrecover_batch_dev(c, d_msg, d_sig, n, d_pub, d_addr, d_st, c->stream);
    if (rc) return rc;
    if (pub65_out) HIPCHK(hipMemcpyAsync(pub65_out, d_pub, n * 65, hipMemcpyDeviceToHost, c->stream));
    if (addr20_out) HIPCHK(hipMemcpyAsync(addr20_out, d_addr, n * 20, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ ECDSA verification, public-key parsing
int gsv_ecdsa_verify_batch_dev(gsv_ctx* c, const uint8_t* d_msg32, const uint8_t* d_sig64, const uint8_t* d_pub65,
                               const uint8_t* d_publen, size_t n, uint8_t* d_ok, void* stream) {
    if (!c || (n && (!d_msg32 || !d_sig64 || !d_pub65 || !d_publen || !d_ok)) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecverify(d_msg32, d_sig64, d_pub65, d_publen, (uint32_t)n, c->gtab, d_ok, st));
}

int gsv_pubkey_parse_batch_dev(gsv_ctx* c, const uint8_t* d_pub65, const uint8_t* d_publen, size_t n,
                               uint8_t* d_pub65_out, uint8_t* d_ok, void* stream) {
    if (!c || (n && (!d_pub65 || !d_publen || !d_pub65_out || !d_ok)) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_pubkey_parse(d_pub65, d_publen, (uint32_t)n, d_pub65_out, d_ok, st));
}

// the offset table of a host form: ascending, and a buffer behind any key that has bytes
static bool key_offsets_ok(const uint8_t* pub, const uint64_t* off, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return false;
    return off[n] == off[0] || pub;
}

int gsv_ecdsa_verify_batch(gsv_ctx* c, const uint8_t* msg32, const uint8_t* sig64, const uint8_t* pub,
                           const uint64_t* pub_off, size_t n, uint8_t* ok) {
    if (!c || (n && (!msg32 || !sig64 || !pub_off || !ok)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!key_offsets_ok(pub, pub_off, n)) return GSV_E_INVALID_ARG;
    std::vector<uint8_t> rows(n * 65), len(n);
    gsv::pubkey_pack(pub, pub_off, n, rows.data(), len.data());
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const VerifyStage p(L, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_msg = p.msg(c->arena), *d_sig = p.sig(c->arena), *d_pub = p.pub(c->arena);
    uint8_t *d_len = p.len(c->arena), *d_ok = p.ok(c->arena);
    HIPCHK(hipMemcpyAsync(d_msg, msg32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_sig, sig64, n * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_pub, rows.data(), n * 65, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_len, len.data(), n, hipMemcpyHostToDevice, c->stream));
    rc = gsv_ecdsa_verify_batch_dev(c, d_msg, d_sig, d_pub, d_len, n, d_ok, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

int gsv_pubkey_parse_batch(gsv_ctx* c, const uint8_t* pub, const uint64_t* pub_off, size_t n, uint8_t* pub65_out,
                           uint8_t* ok) {
    if (!c || (n && (!pub_off || !pub65_out || !ok)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!key_offsets_ok(pub, pub_off, n)) return GSV_E_INVALID_ARG;
    std::vector<uint8_t> rows(n * 65), len(n);
    gsv::pubkey_pack(pub, pub_off, n, rows.data(), len.data());
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const PubkeyParseStage p(L, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_pub = p.pub(c->arena), *d_len = p.len(c->arena), *d_out = p.out(c->arena), *d_ok = p.ok(c->arena);
    HIPCHK(hipMemcpyAsync(d_pub, rows.data(), n * 65, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_len, len.data(), n, hipMemcpyHostToDevice, c->stream));
    rc = gsv_pubkey_parse_batch_dev(c, d_pub, d_len, n, d_out, d_ok, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(pub65_out, d_out, n * 65, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ crypto.Sign, public-key derivation
int gsv_ecdsa_sign_batch_dev(gsv_ctx* c, const uint8_t* d_msg32, const uint8_t* d_seckey32, size_t n,
                             uint8_t* d_sig65_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_msg32 || !d_seckey32 || !d_sig65_out || !d_status)) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecsign(d_msg32, d_seckey32, (uint32_t)n, c->gtab, d_sig65_out, d_status, st));
}

int gsv_pubkey_create_batch_dev(gsv_ctx* c, const uint8_t* d_seckey32, size_t n, uint8_t* d_pub65_out,
                                uint8_t* d_addr20_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_seckey32 || !d_pub65_out || !d_status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_pubkey_create(d_seckey32, (uint32_t)n, c->gtab, d_pub65_out, d_addr20_out, d_status,
                                             st));
}

int gsv_ecdsa_sign_batch(gsv_ctx* c, const uint8_t* msg32, const uint8_t* seckey32, size_t n, uint8_t* sig65_out,
                         uint8_t* status) {
    if (!c || (n && (!msg32 || !seckey32 || !sig65_out || !status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const SignStage p(L, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_key = p.key(c->arena), *d_msg = p.msg(c->arena), *d_sig = p.sig(c->arena), *d_st = p.st(c->arena);
    SecretWipe wipe{c, d_key, n * 32};  // from here on the keys may be in HBM
    HIPCHK(hipMemcpyAsync(d_key, seckey32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_msg, msg32, n * 32, hipMemcpyHostToDevice, c->stream));
    rc = gsv_ecdsa_sign_batch_dev(c, d_msg, d_key, n, d_sig, d_st, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(sig65_out, d_sig, n * 65, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    return wipe.finish();
}

int gsv_pubkey_create_batch(gsv_ctx* c, const uint8_t* seckey32, size_t n, uint8_t* pub65_out, uint8_t* addr20_out,
                            uint8_t* status) {
    if (!c || (n && (!seckey32 || !pub65_out || !status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const PubkeyCreateStage p(L, n, addr20_out != nullptr);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_key = p.key(c->arena), *d_pub = p.pub(c->arena), *d_st = p.st(c->arena);
    uint8_t* d_addr = p.addr(c->arena);  // nullptr when not asked for
    SecretWipe wipe{c, d_key, n * 32};
    HIPCHK(hipMemcpyAsync(d_key, seckey32, n * 32, hipMemcpyHostToDevice, c->stream));
    rc = gsv_pubkey_create_batch_dev(c, d_key, n, d_pub, d_addr, d_st, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(pub65_out, d_pub, n * 65, hipMemcpyDeviceToHost, c->stream));
    if (addr20_out) HIPCHK(hipMemcpyAsync(addr20_out, d_addr, n * 20, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    return wipe.finish();
}

// ------------------------------------------------------------------ ScalarMult, ECDH (crypto/secp256k1/ext.h:104-142)
int gsv_secp256k1_scalar_mul_batch_dev(gsv_ctx* c, const uint8_t* d_point64, const uint8_t* d_scalar32, size_t n,
                                       uint8_t* d_point64_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_point64 || !d_scalar32 || !d_point64_out || !d_status)) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecdh(d_point64, d_scalar32, (uint32_t)n, d_point64_out, nullptr, nullptr, d_status, st));
}

int gsv_ecdh_batch_dev(gsv_ctx* c, const uint8_t* d_pub64, const uint8_t* d_seckey32, size_t n,
                       uint8_t* d_shared32_out, uint8_t* d_keys48_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_pub64 || !d_seckey32 || !d_status || (!d_shared32_out && !d_keys48_out))) ||
        n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecdh(d_pub64, d_seckey32, (uint32_t)n, nullptr, d_shared32_out, d_keys48_out, d_status,
                                    st));
}

int gsv_secp256k1_scalar_mul_batch(gsv_ctx* c, const uint8_t* point64, const uint8_t* scalar32, size_t n,
                                   uint8_t* point64_out, uint8_t* status) {
    if (!c || (n && (!point64 || !scalar32 || !point64_out || !status)) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const ScalarMulStage p(L, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_key = p.key(c->arena), *d_out = p.out(c->arena), *d_pt = p.pt(c->arena), *d_st = p.st(c->arena);
    SecretWipe wipe{c, c->arena, p.secret};  // the scalars and the product points
    HIPCHK(hipMemcpyAsync(d_key, scalar32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_pt, point64, n * 64, hipMemcpyHostToDevice, c->stream));
    rc = gsv_secp256k1_scalar_mul_batch_dev(c, d_pt, d_key, n, d_out, d_st, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(point64_out, d_out, n * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    return wipe.finish();
}

int gsv_ecdh_batch(gsv_ctx* c, const uint8_t* pub64, const uint8_t* seckey32, size_t n, uint8_t* shared32_out,
                   uint8_t* keys48_out, uint8_t* status) {
    if (!c || (n && (!pub64 || !seckey32 || !status || (!shared32_out && !keys48_out))) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const EcdhStage p(L, n, shared32_out != nullptr, keys48_out != nullptr);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_key = p.key(c->arena), *d_pt = p.pt(c->arena), *d_st = p.st(c->arena);
    uint8_t *d_sh = p.shared(c->arena), *d_keys = p.keys(c->arena);  // nullptr when not asked for
    SecretWipe wipe{c, c->arena, p.secret};  // the secret keys, the shared secrets, the derived keys
    HIPCHK(hipMemcpyAsync(d_key, seckey32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_pt, pub64, n * 64, hipMemcpyHostToDevice, c->stream));
    rc = gsv_ecdh_batch_dev(c, d_pt, d_key, n, d_sh, d_keys, d_st, c->stream);
    if (rc) return rc;
    if (shared32_out) HIPCHK(hipMemcpyAsync(shared32_out, d_sh, n * 32, hipMemcpyDeviceToHost, c->stream));
    if (keys48_out) HIPCHK(hipMemcpyAsync(keys48_out, d_keys, n * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    return wipe.finish();
}

// Test hook of the rule above: bytes [off, off + n) of the context's staging arena, as they are now.
int gsv_ctx_arena_read(gsv_ctx* c, size_t off, size_t n, uint8_t* out) {
    if (!c || (n && !out)) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (off > c->arena_cap || n > c->arena_cap - off) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, c->arena + off, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ ecrecover precompile (contracts.go:78-101)
int gsv_ecrecover_precompile_batch_dev(gsv_ctx* c, const uint8_t* d_in128, size_t n, uint8_t* d_out32, uint8_t* d_ok,
                                       void* stream) {
    if (!c || (n && (!d_in128 || !d_out32 || !d_ok)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecrecover_precompile(d_in128, (uint32_t)n, c->gtab, d_out32, d_ok, st));
}

int gsv_ecrecover_precompile_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out32,
                                   uint8_t* ok) {
    if (!c || (n && (!off || !out32 || !ok)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return GSV_E_INVALID_ARG;
    if (off[n] > off[0] && !in) return GSV_E_INVALID_ARG;
    // common.RightPadBytes(input, 128); only input[0:128] is read (contracts.go:81-90)
    std::vector<uint8_t> pad(n * 128, 0);
    for (size_t i = 0; i < n; i++) {
        size_t len = std::min<uint64_t>(off[i + 1] - off[i], 128);
        if (len) memcpy(&pad[i * 128], in + off[i], len);
    }
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const RecordStage p(L, n, 128, 32);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t* d_in = p.in(c->arena);
    uint8_t* d_out = p.out(c->arena);
    uint8_t* d_ok = p.st(c->arena);
    HIPCHK(hipMemcpyAsync(d_in, pad.data(), n * 128, hipMemcpyHostToDevice, c->stream));
    rc = gsv_ecrecover_precompile_batch_dev(c, d_in, n, d_out, d_ok, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out32, d_out, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ bn256Add / bn256ScalarMul (contracts.go:274-312)
// GSV_BN_G1_BITSERIAL=1 selects the bit-serial multiplication kernel (A/B timing and the tests only)
static int bn_g1_bitserial() {
    const char* e = getenv("GSV_BN_G1_BITSERIAL");
    return e && atoi(e) != 0;
}

int gsv_bn256_add_batch_dev(gsv_ctx* c, const uint8_t* d_in128, size_t n, uint8_t* d_out64, uint8_t* d_status,
                            void* stream) {
    if (!c || (n && (!d_in128 || !d_out64 || !d_status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_BN_G1, st);
    return hip_err(gsv::launch_bn256_g1_add(d_in128, (uint32_t)n, d_out64, d_status, st));
}

int gsv_bn256_scalar_mul_batch_dev(gsv_ctx* c, const uint8_t* d_in96, size_t n, uint8_t* d_out64, uint8_t* d_status,
                                   void* stream) {
    if (!c || (n && (!d_in96 || !d_out64 || !d_status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    KTimer t(c, GSV_K_BN_G1, st);
    return hip_err(gsv::launch_bn256_g1_mul(d_in96, (uint32_t)n, d_out64, d_status, bn_g1_bitserial(), st));
}

// getData(input, 0, rec) (core/vm/common.go:37-47): right-pad with zeros, ignore what follows; stage,
// launch, copy back
static int bn_g1_host(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, size_t rec, uint8_t* out64,
                      uint8_t* status) {
    if (!c || (n && (!off || !out64 || !status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return GSV_E_INVALID_ARG;
    if (off[n] > off[0] && !in) return GSV_E_INVALID_ARG;
    std::vector<uint8_t> pad(n * rec, 0);
    for (size_t i = 0; i < n; i++) {
        size_t len = std::min<uint64_t>(off[i + 1] - off[i], rec);
        if (len) memcpy(&pad[i * rec], in + off[i], len);
    }
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const RecordStage p(L, n, rec, 64);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t* d_in = p.in(c->arena);
    uint8_t* d_out = p.out(c->arena);
    uint8_t* d_st = p.st(c->arena);
    HIPCHK(hipMemcpyAsync(d_in, pad.data(), n * rec, hipMemcpyHostToDevice, c->stream));
    rc = rec == 128 ? gsv_bn256_add_batch_dev(c, d_in, n, d_out, d_st, c->stream)
                    : gsv_bn256_scalar_mul_batch_dev(c, d_in, n, d_out, d_st, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out64, d_out, n * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

int gsv_bn256_add_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out64,
                        uint8_t* status) {
    return bn_g1_host(c, in, off, n, 128, out64, status);
}

int gsv_bn256_scalar_mul_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out64,
                               uint8_t* status) {
    return bn_g1_host(c, in, off, n, 96, out64, status);
}

// ------------------------------------------------------------------ recoverPlain
int gsv_sender_batch(gsv_ctx* c, const uint8_t* sighash32, const uint8_t* r32, const uint8_t* s32,
                     const uint64_t* v, const uint8_t* v_big, size_t n, int homestead,
                     uint8_t* addr20_out, uint8_t* status) {
    if (!c || (n && (!sighash32 || !r32 || !s32 || !v || !v_big || !addr20_out || !status)) ||
        n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const SenderStage p(L, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_h = p.h(c->arena), *d_r = p.r(c->arena), *d_s = p.s(c->arena);
    uint64_t* d_v = p.v(c->arena);
    uint8_t *d_vb = p.vb(c->arena), *d_a = p.a(c->arena), *d_st = p.st(c->arena);
    HIPCHK(hipMemcpyAsync(d_h, sighash32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_r, r32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_s, s32, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_v, v, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_vb, v_big, n, hipMemcpyHostToDevice, c->stream));
    {
        KTimer t(c, GSV_K_ECRECOVER, c->stream);
        HIPCHK(gsv::launch_sender(d_h, d_r, d_s, d_v, d_vb, (uint32_t)n, homestead, c->gtab, d_a, d_st,
                                  c->stream));
    }
    HIPCHK(hipMemcpyAsync(addr20_out, d_a, n * 20, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ synthetic signer (bench data)
int gsv_synth_sign_dev(gsv_ctx* c, uint64_t seed, size_t n, uint8_t* d_msg32, uint8_t* d_sig65,
                       uint8_t* d_pub65, uint8_t* d_addr20, void* stream) {
    if (!c || (n && (!d_msg32 || !d_sig65)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return hip_err(gsv::launch_synth_sign(seed, (uint32_t)n, c->gtab, d_msg32, d_sig65, d_pub65,
                                          d_addr20, st));
}

int gsv_synth_sign(gsv_ctx* c, uint64_t seed, size_t n, uint8_t* msg32, uint8_t* sig65,
                   uint8_t* pub65, uint8_t* addr20) {
    if (!c || (n && (!msg32 || !sig65)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const SynthSignStage p(L, n, pub65 != nullptr, addr20 != nullptr);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_m = p.msg(c->arena), *d_s = p.sig(c->arena);
    uint8_t *d_p = p.pub(c->arena), *d_a = p.addr(c->arena);  // nullptr when not asked for
    rc = gsv_synth_sign_dev(c, seed, n, d_m, d_s, d_p, d_a, c->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(msg32, d_m, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sig65, d_s, n * 65, hipMemcpyDeviceToHost, c->stream));
    if (pub65) HIPCHK(hipMemcpyAsync(pub65, d_p, n * 65, hipMemcpyDeviceToHost, c->stream));
    if (addr20) HIPCHK(hipMemcpyAsync(addr20, d_a, n * 20, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ types.Sender over tx RLP
// Host: decode + sighash preimages (threads). GPU: Keccak of the preimages, recoverPlain + address.
static int tx_sender_impl(gsv_ctx* c, const uint8_t* rlp, const uint64_t* off, size_t n, const uint8_t* cid,
                          size_t cidlen, int signer_kind, uint8_t* addr_out, uint8_t* status_out) {
    std::vector<uint8_t> hst(n), rr(n * 32), ss(n * 32), vb(n);
    std::vector<uint64_t> vv(n), plen(n);
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < 4096) nt = 1;
    std::vector<std::vector<uint8_t>> tpre(nt);
    std::vector<std::thread> th;
    auto work = [&](unsigned t) {
        size_t lo = n * t / nt, hi = n * (t + 1) / nt;
        gsv::TxPrep p;
        for (size_t i = lo; i < hi; i++) {
            int st = gsv::tx_prepare(rlp + off[i], off[i + 1] - off[i], cid, cidlen, signer_kind, p);
            hst[i] = (uint8_t)st;
            if (st != GSV_ST_OK) {
                plen[i] = 0;
                vb[i] = 1;
                continue;
            }
            memcpy(&rr[i * 32], p.r32, 32);
            memcpy(&ss[i * 32], p.s32, 32);
            vv[i] = p.v;
            vb[i] = p.vbig;
            plen[i] = p.pre.size();
            tpre[t].insert(tpre[t].end(), p.pre.begin(), p.pre.end());
        }
    };
    for (unsigned t = 0; t < nt; t++) th.emplace_back(work, t);
    for (auto& x : th) x.join();
    std::vector<uint64_t> poff(n + 1);
    poff[0] = 0;
    for (size_t i = 0; i < n; i++) poff[i + 1] = poff[i] + plen[i];
    size_t pbytes = poff[n];
    int homestead = signer_kind == GSV_SIGNER_FRONTIER ? 0 : 1;
    Layout L;
    const TxSenderStage p(L, pbytes, n);
    int rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t* d_pre = p.pre(c->arena);
    uint64_t* d_poff = p.poff(c->arena);
    uint8_t *d_h = p.snd.h(c->arena), *d_r = p.snd.r(c->arena), *d_s = p.snd.s(c->arena);
    uint64_t* d_v = p.snd.v(c->arena);
    uint8_t *d_vb = p.snd.vb(c->arena), *d_a = p.snd.a(c->arena), *d_st = p.snd.st(c->arena);
    size_t w = 0;
    for (unsigned t = 0; t < nt; t++) {
        if (!tpre[t].empty())
            HIPCHK(hipMemcpyAsync(d_pre + w, tpre[t].data(), tpre[t].size(), hipMemcpyHostToDevice, c->stream));
        w += tpre[t].size();
    }
    HIPCHK(hipMemcpyAsync(d_poff, poff.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_r, rr.data(), n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_s, ss.data(), n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_v, vv.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_vb, vb.data(), n, hipMemcpyHostToDevice, c->stream));
    {
        KTimer t(c, GSV_K_SENDER_PREP, c->stream);
        HIPCHK(gsv::launch_keccak256(d_pre, d_poff, (uint32_t)n, d_h, c->stream));
    }
    {
        KTimer t(c, GSV_K_ECRECOVER, c->stream);
        HIPCHK(gsv::launch_sender(d_h, d_r, d_s, d_v, d_vb, (uint32_t)n, homestead, c->gtab, d_a, d_st, c->stream));
    }
    HIPCHK(hipMemcpyAsync(addr_out, d_a, n * 20, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++)
        if (hst[i] != GSV_ST_OK) {
            status_out[i] = hst[i];
            memset(addr_out + i * 20, 0, 20);
        }
    return GSV_SUCCESS;
}

int gsv_tx_sender_batch(gsv_ctx* c, const uint8_t* rlp, const uint64_t* off, size_t n, const uint8_t* chain_id,
                        size_t chain_id_len, int signer_kind, uint8_t* addr20_out, uint8_t* status) {
    if (!c || (n && (!rlp || !off || !addr20_out || !status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (signer_kind < GSV_SIGNER_EIP155 || signer_kind > GSV_SIGNER_FRONTIER) return GSV_E_INVALID_ARG;
    if (chain_id_len && !chain_id) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    for (size_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return tx_sender_impl(c, rlp, off, n, chain_id, chain_id_len, signer_kind, addr20_out, status);
}

}  // extern "C"

// ecies.Encrypt / PrivateKey.Decrypt of the C ABI (gsv_ctx.h): the launch chains around the ladder
// (ecies.hip draws them) and the host forms' staging.
#include "gsv_ctx.h"

using namespace gsv::api;

namespace {

// a host form's offset table: ascending, every item below 2^32 bytes, a buffer behind any bytes
int table_check(const void* data, const uint64_t* off, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (off[i + 1] < off[i]) return GSV_E_INVALID_ARG;
        if (off[i + 1] - off[i] > 0xFFFFFFFFull) return GSV_E_TOO_LARGE;
    }
    return off[n] > off[0] && !data ? GSV_E_INVALID_ARG : GSV_SUCCESS;
}

// the table rebased to its first entry, as the staged copy of the bytes is
std::vector<uint64_t> rebased(const uint64_t* off, size_t n) {
    std::vector<uint64_t> rel(n + 1);
    for (size_t i = 0; i <= n; i++) rel[i] = off[i] - off[0];
    return rel;
}

}  // namespace

extern "C" {

size_t gsv_ecies_work_bytes(size_t n, int encrypt) { return n * (encrypt ? gsv::ECIES_WORK_ENC : gsv::ECIES_WORK_DEC); }

int gsv_ecies_decrypt_batch_dev(gsv_ctx* c, const uint8_t* d_ct, const uint64_t* d_ct_off, const uint8_t* d_seckey32,
                                const uint8_t* d_s2, const uint64_t* d_s2_off, size_t n, uint8_t* d_msg_out,
                                uint32_t* d_msg_len, uint8_t* d_status, uint8_t* d_work, void* stream) {
    if (!c || (n && (!d_ct || !d_ct_off || !d_seckey32 || !d_msg_out || !d_msg_len || !d_status || !d_work)) ||
        n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    uint8_t *keys = d_work, *rows = d_work + n * 48, *est = d_work + n * 112;
    {
        KTimer t(c, GSV_K_ECRECOVER, st);
        HIPCHK(gsv::launch_ecies_parse(d_ct, d_ct_off, d_seckey32, (uint32_t)n, rows, d_status, st));
        HIPCHK(gsv::launch_ecdh(rows, d_seckey32, (uint32_t)n, nullptr, nullptr, keys, est, st));
    }
    KTimer t(c, GSV_K_ECIES, st);
    return hip_err(gsv::launch_ecies_open(d_ct, d_ct_off, d_s2, d_s2_off, (uint32_t)n, d_work, d_msg_out, d_msg_len,
                                          d_status, st));
}

int gsv_ecies_encrypt_batch_dev(gsv_ctx* c, const uint8_t* d_msg, const uint64_t* d_msg_off, const uint8_t* d_pub64,
                                const uint8_t* d_eph_seckey32, const uint8_t* d_iv16, const uint8_t* d_s2,
                                const uint64_t* d_s2_off, size_t n, uint8_t* d_ct_out, uint8_t* d_status, uint8_t* d_work,
                                void* stream) {
    if (!c ||
        (n && (!d_msg || !d_msg_off || !d_pub64 || !d_eph_seckey32 || !d_iv16 || !d_ct_out || !d_status || !d_work)) ||
        n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    uint8_t *keys = d_work, *rows = d_work + n * 48, *est = d_work + n * 113, *pst = d_work + n * 114;
    {
        KTimer t(c, GSV_K_ECRECOVER, st);
        HIPCHK(gsv::launch_pubkey_create(d_eph_seckey32, (uint32_t)n, c->gtab, rows, nullptr, pst, st));
        HIPCHK(gsv::launch_ecdh(d_pub64, d_eph_seckey32, (uint32_t)n, nullptr, nullptr, keys, est, st));
    }
    KTimer t(c, GSV_K_ECIES, st);
    return hip_err(gsv::launch_ecies_seal(d_msg, d_msg_off, d_iv16, d_s2, d_s2_off, (uint32_t)n, d_work, d_ct_out,
                                          d_status, st));
}

int gsv_ecies_decrypt_batch(gsv_ctx* c, const uint8_t* ct, const uint64_t* ct_off, const uint8_t* seckey32,
                            const uint8_t* s2, const uint64_t* s2_off, size_t n, uint8_t* msg_out, uint32_t* msg_len,
                            uint8_t* status) {
    if (!c || (n && (!ct_off || !seckey32 || !msg_len || !status)) || n > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = table_check(ct, ct_off, n);
    if (rc) return rc;
    const size_t bytes = ct_off[n] - ct_off[0];
    if (bytes && !msg_out) return GSV_E_INVALID_ARG;
    if (s2_off && (rc = table_check(s2, s2_off, n))) return rc;
    const size_t s2_bytes = s2_off ? s2_off[n] - s2_off[0] : 0;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const EciesDecryptStage p(L, n, gsv::ECIES_WORK_DEC, bytes, s2_bytes, s2_off != nullptr);
    rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_key = p.key(c->arena), *d_work = p.work(c->arena), *d_msg = p.msg(c->arena), *d_ct = p.ct(c->arena);
    uint8_t *d_s2 = p.s2(c->arena), *d_st = p.st(c->arena);  // d_s2, d_s2off: nullptr without a table
    uint64_t *d_off = p.off(c->arena), *d_s2off = p.s2off(c->arena);
    uint32_t* d_mlen = p.mlen(c->arena);
    SecretWipe wipe{c, c->arena, p.secret};  // the secret keys, Ke || Km, the plaintext
    const std::vector<uint64_t> rel = rebased(ct_off, n);
    std::vector<uint64_t> s2rel;
    HIPCHK(hipMemcpyAsync(d_key, seckey32, n * 32, hipMemcpyHostToDevice, c->stream));
    if (bytes) HIPCHK(hipMemcpyAsync(d_ct, ct + ct_off[0], bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (s2_off) {
        s2rel = rebased(s2_off, n);
        if (s2_bytes) HIPCHK(hipMemcpyAsync(d_s2, s2 + s2_off[0], s2_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_s2off, s2rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    }
    rc = gsv_ecies_decrypt_batch_dev(c, d_ct, d_off, d_key, d_s2, d_s2off, n, d_msg, d_mlen, d_st, d_work, c->stream);
    if (rc) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(msg_out + ct_off[0], d_msg, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(msg_len, d_mlen, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    return wipe.finish();
}

int gsv_ecies_encrypt_batch(gsv_ctx* c, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* pub64,
                            const uint8_t* eph_seckey32, const uint8_t* iv16, const uint8_t* s2, const uint64_t* s2_off,
                            size_t n, uint8_t* ct_out, uint8_t* status) {
    if (!c || (n && (!msg_off || !pub64 || !eph_seckey32 || !iv16 || !ct_out || !status)) || n > 0xFFFFFFFFull)
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = table_check(msg, msg_off, n);
    if (rc) return rc;
    const size_t bytes = msg_off[n] - msg_off[0];
    if (s2_off && (rc = table_check(s2, s2_off, n))) return rc;
    const size_t s2_bytes = s2_off ? s2_off[n] - s2_off[0] : 0;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Layout L;
    const EciesEncryptStage p(L, n, gsv::ECIES_WORK_ENC, bytes, s2_bytes, s2_off != nullptr);
    rc = arena_reserve(c, L.n);
    if (rc) return rc;
    uint8_t *d_key = p.key(c->arena), *d_work = p.work(c->arena), *d_msg = p.msg(c->arena), *d_pub = p.pub(c->arena);
    uint8_t *d_iv = p.iv(c->arena), *d_s2 = p.s2(c->arena), *d_ct = p.ct(c->arena), *d_st = p.st(c->arena);
    uint64_t *d_off = p.off(c->arena), *d_s2off = p.s2off(c->arena);
    SecretWipe wipe{c, c->arena, p.secret};  // the ephemeral keys, Ke || Km, the plaintext
    const std::vector<uint64_t> rel = rebased(msg_off, n);
    std::vector<uint64_t> s2rel;
    HIPCHK(hipMemcpyAsync(d_key, eph_seckey32, n * 32, hipMemcpyHostToDevice, c->stream));
    if (bytes) HIPCHK(hipMemcpyAsync(d_msg, msg + msg_off[0], bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_pub, pub64, n * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_iv, iv16, n * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_off, rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (s2_off) {
        s2rel = rebased(s2_off, n);
        if (s2_bytes) HIPCHK(hipMemcpyAsync(d_s2, s2 + s2_off[0], s2_bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_s2off, s2rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    }
    rc = gsv_ecies_encrypt_batch_dev(c, d_msg, d_off, d_pub, d_key, d_iv, d_s2, d_s2off, n, d_ct, d_st, d_work, c->stream);
    if (rc) return rc;
    // item i at ct_out + msg_off[i] + 113 i: the staged table starts at 0, the caller's at msg_off[0]
    HIPCHK(hipMemcpyAsync(ct_out + msg_off[0], d_ct, bytes + n * GSV_ECIES_OVERHEAD, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, c->stream));
    return wipe.finish();
}

}  // extern "C"

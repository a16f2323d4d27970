// ecies.Encrypt / PrivateKey.Decrypt of the C ABI (gsv_ctx.h): the launch chains around the ladder
// (ecies.hip draws them) and the host forms' staging.
#include "gsv_ctx.h"

using namespace gsv::api;

extern "C" {

size_t gsv_ecies_work_bytes(size_t n, int encrypt) { return n * (encrypt ? gsv::ECIES_WORK_ENC : gsv::ECIES_WORK_DEC); }

int gsv_ecies_decrypt_batch_dev(gsv_ctx* c, const uint8_t* d_ct, const uint64_t* d_ct_off, const uint8_t* d_seckey32,
                                const uint8_t* d_s2, const uint64_t* d_s2_off, size_t n, uint8_t* d_msg_out,
                                uint32_t* d_msg_len, uint8_t* d_status, uint8_t* d_work, void* stream) {
    if (!c || (n && (!d_ct || !d_ct_off || !d_seckey32 || !d_msg_out || !d_msg_len || !d_status || !d_work)) ||
        batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream_of(c, stream);
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
        batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream_of(c, stream);
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
    if (!c || (n && (!ct_off || !seckey32 || !msg_len || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(ct, ct_off, n, kBelow4G));
    const size_t bytes = ct_off[n] - ct_off[0];
    if (bytes && !msg_out) return GSV_E_INVALID_ARG;
    if (s2_off) GSVCHK(table_check(s2, s2_off, n, kBelow4G));
    const size_t s2_bytes = s2_off ? s2_off[n] - s2_off[0] : 0;
    const std::vector<uint64_t> rel = table_rebase(ct_off, n);
    const std::vector<uint64_t> s2rel = s2_off ? table_rebase(s2_off, n) : std::vector<uint64_t>();
    Layout L;
    const EciesDecryptStage p(L, n, gsv::ECIES_WORK_DEC, bytes, s2_bytes, s2_off != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.secret);  // the secret keys, Ke || Km, the plaintext
    GSVCHK(s.in(p.key, seckey32));
    GSVCHK(s.in(p.ct, ct + ct_off[0]));
    GSVCHK(s.in(p.off, rel.data()));
    if (s2_off) {  // p.s2, p.s2off: absent without a table
        GSVCHK(s.in(p.s2, s2 + s2_off[0]));
        GSVCHK(s.in(p.s2off, s2rel.data()));
    }
    GSVCHK(gsv_ecies_decrypt_batch_dev(c, s(p.ct), s(p.off), s(p.key), s(p.s2), s(p.s2off), n, s(p.msg), s(p.mlen),
                                       s(p.st), s(p.work), c->stream));
    GSVCHK(s.out(msg_out + ct_off[0], p.msg));
    GSVCHK(s.out(msg_len, p.mlen));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

int gsv_ecies_encrypt_batch(gsv_ctx* c, const uint8_t* msg, const uint64_t* msg_off, const uint8_t* pub64,
                            const uint8_t* eph_seckey32, const uint8_t* iv16, const uint8_t* s2, const uint64_t* s2_off,
                            size_t n, uint8_t* ct_out, uint8_t* status) {
    if (!c || (n && (!msg_off || !pub64 || !eph_seckey32 || !iv16 || !ct_out || !status)) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(msg, msg_off, n, kBelow4G));
    const size_t bytes = msg_off[n] - msg_off[0];
    if (s2_off) GSVCHK(table_check(s2, s2_off, n, kBelow4G));
    const size_t s2_bytes = s2_off ? s2_off[n] - s2_off[0] : 0;
    const std::vector<uint64_t> rel = table_rebase(msg_off, n);
    const std::vector<uint64_t> s2rel = s2_off ? table_rebase(s2_off, n) : std::vector<uint64_t>();
    Layout L;
    const EciesEncryptStage p(L, n, gsv::ECIES_WORK_ENC, bytes, s2_bytes, s2_off != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.secret);  // the ephemeral keys, Ke || Km, the plaintext
    GSVCHK(s.in(p.key, eph_seckey32));
    GSVCHK(s.in(p.msg, msg + msg_off[0]));
    GSVCHK(s.in(p.pub, pub64));
    GSVCHK(s.in(p.iv, iv16));
    GSVCHK(s.in(p.off, rel.data()));
    if (s2_off) {  // p.s2, p.s2off: absent without a table
        GSVCHK(s.in(p.s2, s2 + s2_off[0]));
        GSVCHK(s.in(p.s2off, s2rel.data()));
    }
    GSVCHK(gsv_ecies_encrypt_batch_dev(c, s(p.msg), s(p.off), s(p.pub), s(p.key), s(p.iv), s(p.s2), s(p.s2off), n,
                                       s(p.ct), s(p.st), s(p.work), c->stream));
    // item i at ct_out + msg_off[i] + 113 i: the staged table starts at 0, the caller's at msg_off[0]
    GSVCHK(s.out(ct_out + msg_off[0], p.ct));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

}  // extern "C"

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
    if (!c || (n && (!d_off || !d_out32)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_KECCAK, st);
    return hip_err(gsv::launch_keccak256(d_data, d_off, (uint32_t)n, d_out32, st));
}

int gsv_keccak256_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n,
                        uint8_t* out32) {
    return hash_host(c, GSV_K_KECCAK, gsv::launch_keccak256, data, off, n, out32);
}

// ------------------------------------------------------------------ ecrecover
int gsv_ecrecover_batch_dev(gsv_ctx* c, const uint8_t* d_msg32, const uint8_t* d_sig65, size_t n,
                            uint8_t* d_pub65, uint8_t* d_addr20, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_msg32 || !d_sig65 || !d_status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecrecover(d_msg32, d_sig65, (uint32_t)n, c->gtab, d_pub65, d_addr20,
                                         d_status, st));
}

int gsv_ecrecover_batch(gsv_ctx* c, const uint8_t* msg32, const uint8_t* sig65, size_t n,
                        uint8_t* pub65_out, uint8_t* addr20_out, uint8_t* status) {
    if (!c || (n && (!msg32 || !sig65 || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const EcrecoverStage p(L, n, pub65_out != nullptr, addr20_out != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.msg, msg32));
    GSVCHK(s.in(p.sig, sig65));
    // s(p.pub), s(p.addr): nullptr when not asked for
    GSVCHK(gsv_ecrecover_batch_dev(c, s(p.msg), s(p.sig), n, s(p.pub), s(p.addr), s(p.st), c->stream));
    GSVCHK(s.out(pub65_out, p.pub));
    GSVCHK(s.out(addr20_out, p.addr));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

// ------------------------------------------------------------------ ECDSA verification, public-key parsing
int gsv_ecdsa_verify_batch_dev(gsv_ctx* c, const uint8_t* d_msg32, const uint8_t* d_sig64, const uint8_t* d_pub65,
                               const uint8_t* d_publen, size_t n, uint8_t* d_ok, void* stream) {
    if (!c || (n && (!d_msg32 || !d_sig64 || !d_pub65 || !d_publen || !d_ok)) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecverify(d_msg32, d_sig64, d_pub65, d_publen, (uint32_t)n, c->gtab, d_ok, st));
}

int gsv_pubkey_parse_batch_dev(gsv_ctx* c, const uint8_t* d_pub65, const uint8_t* d_publen, size_t n,
                               uint8_t* d_pub65_out, uint8_t* d_ok, void* stream) {
    if (!c || (n && (!d_pub65 || !d_publen || !d_pub65_out || !d_ok)) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_pubkey_parse(d_pub65, d_publen, (uint32_t)n, d_pub65_out, d_ok, st));
}

int gsv_ecdsa_verify_batch(gsv_ctx* c, const uint8_t* msg32, const uint8_t* sig64, const uint8_t* pub,
                           const uint64_t* pub_off, size_t n, uint8_t* ok) {
    if (!c || (n && (!msg32 || !sig64 || !pub_off || !ok)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(pub, pub_off, n));
    std::vector<uint8_t> rows(n * 65), len(n);
    gsv::pubkey_pack(pub, pub_off, n, rows.data(), len.data());
    Layout L;
    const VerifyStage p(L, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.msg, msg32));
    GSVCHK(s.in(p.sig, sig64));
    GSVCHK(s.in(p.pub, rows.data()));
    GSVCHK(s.in(p.len, len.data()));
    GSVCHK(gsv_ecdsa_verify_batch_dev(c, s(p.msg), s(p.sig), s(p.pub), s(p.len), n, s(p.ok), c->stream));
    GSVCHK(s.out(ok, p.ok));
    return s.finish();
}

int gsv_pubkey_parse_batch(gsv_ctx* c, const uint8_t* pub, const uint64_t* pub_off, size_t n, uint8_t* pub65_out,
                           uint8_t* ok) {
    if (!c || (n && (!pub_off || !pub65_out || !ok)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(pub, pub_off, n));
    std::vector<uint8_t> rows(n * 65), len(n);
    gsv::pubkey_pack(pub, pub_off, n, rows.data(), len.data());
    Layout L;
    const PubkeyParseStage p(L, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.pub, rows.data()));
    GSVCHK(s.in(p.len, len.data()));
    GSVCHK(gsv_pubkey_parse_batch_dev(c, s(p.pub), s(p.len), n, s(p.out), s(p.ok), c->stream));
    GSVCHK(s.out(pub65_out, p.out));
    GSVCHK(s.out(ok, p.ok));
    return s.finish();
}

// ------------------------------------------------------------------ crypto.Sign, public-key derivation
int gsv_ecdsa_sign_batch_dev(gsv_ctx* c, const uint8_t* d_msg32, const uint8_t* d_seckey32, size_t n,
                             uint8_t* d_sig65_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_msg32 || !d_seckey32 || !d_sig65_out || !d_status)) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecsign(d_msg32, d_seckey32, (uint32_t)n, c->gtab, d_sig65_out, d_status, st));
}

int gsv_pubkey_create_batch_dev(gsv_ctx* c, const uint8_t* d_seckey32, size_t n, uint8_t* d_pub65_out,
                                uint8_t* d_addr20_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_seckey32 || !d_pub65_out || !d_status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_pubkey_create(d_seckey32, (uint32_t)n, c->gtab, d_pub65_out, d_addr20_out, d_status,
                                             st));
}

int gsv_ecdsa_sign_batch(gsv_ctx* c, const uint8_t* msg32, const uint8_t* seckey32, size_t n, uint8_t* sig65_out,
                         uint8_t* status) {
    if (!c || (n && (!msg32 || !seckey32 || !sig65_out || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const SignStage p(L, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.key);  // from here on the keys may be in HBM
    GSVCHK(s.in(p.key, seckey32));
    GSVCHK(s.in(p.msg, msg32));
    GSVCHK(gsv_ecdsa_sign_batch_dev(c, s(p.msg), s(p.key), n, s(p.sig), s(p.st), c->stream));
    GSVCHK(s.out(sig65_out, p.sig));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

int gsv_pubkey_create_batch(gsv_ctx* c, const uint8_t* seckey32, size_t n, uint8_t* pub65_out, uint8_t* addr20_out,
                            uint8_t* status) {
    if (!c || (n && (!seckey32 || !pub65_out || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const PubkeyCreateStage p(L, n, addr20_out != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.key);
    GSVCHK(s.in(p.key, seckey32));
    GSVCHK(gsv_pubkey_create_batch_dev(c, s(p.key), n, s(p.pub), s(p.addr), s(p.st), c->stream));
    GSVCHK(s.out(pub65_out, p.pub));
    GSVCHK(s.out(addr20_out, p.addr));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

// ------------------------------------------------------------------ ScalarMult, ECDH (crypto/secp256k1/ext.h:104-142)
int gsv_secp256k1_scalar_mul_batch_dev(gsv_ctx* c, const uint8_t* d_point64, const uint8_t* d_scalar32, size_t n,
                                       uint8_t* d_point64_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_point64 || !d_scalar32 || !d_point64_out || !d_status)) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecdh(d_point64, d_scalar32, (uint32_t)n, d_point64_out, nullptr, nullptr, d_status, st));
}

int gsv_ecdh_batch_dev(gsv_ctx* c, const uint8_t* d_pub64, const uint8_t* d_seckey32, size_t n,
                       uint8_t* d_shared32_out, uint8_t* d_keys48_out, uint8_t* d_status, void* stream) {
    if (!c || (n && (!d_pub64 || !d_seckey32 || !d_status || (!d_shared32_out && !d_keys48_out))) ||
        batch_too_long(n))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecdh(d_pub64, d_seckey32, (uint32_t)n, nullptr, d_shared32_out, d_keys48_out, d_status,
                                    st));
}

int gsv_secp256k1_scalar_mul_batch(gsv_ctx* c, const uint8_t* point64, const uint8_t* scalar32, size_t n,
                                   uint8_t* point64_out, uint8_t* status) {
    if (!c || (n && (!point64 || !scalar32 || !point64_out || !status)) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const ScalarMulStage p(L, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.secret);  // the scalars and the product points
    GSVCHK(s.in(p.key, scalar32));
    GSVCHK(s.in(p.pt, point64));
    GSVCHK(gsv_secp256k1_scalar_mul_batch_dev(c, s(p.pt), s(p.key), n, s(p.out), s(p.st), c->stream));
    GSVCHK(s.out(point64_out, p.out));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

int gsv_ecdh_batch(gsv_ctx* c, const uint8_t* pub64, const uint8_t* seckey32, size_t n, uint8_t* shared32_out,
                   uint8_t* keys48_out, uint8_t* status) {
    if (!c || (n && (!pub64 || !seckey32 || !status || (!shared32_out && !keys48_out))) || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const EcdhStage p(L, n, shared32_out != nullptr, keys48_out != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.secret);  // the secret keys, the shared secrets, the derived keys
    GSVCHK(s.in(p.key, seckey32));
    GSVCHK(s.in(p.pt, pub64));
    GSVCHK(gsv_ecdh_batch_dev(c, s(p.pt), s(p.key), n, s(p.shared), s(p.keys), s(p.st), c->stream));
    GSVCHK(s.out(shared32_out, p.shared));
    GSVCHK(s.out(keys48_out, p.keys));
    GSVCHK(s.out(status, p.st));
    return s.finish();
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
    if (!c || (n && (!d_in128 || !d_out32 || !d_ok)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_ECRECOVER, st);
    return hip_err(gsv::launch_ecrecover_precompile(d_in128, (uint32_t)n, c->gtab, d_out32, d_ok, st));
}

// A precompile over fixed records: common.RightPadBytes(input, rec) / getData(input, 0, rec), of which only
// input[0:rec] is read (contracts.go:81-90, core/vm/common.go:37-47); stage, launch, copy back
typedef int (*record_dev)(gsv_ctx*, const uint8_t*, size_t, uint8_t*, uint8_t*, void*);

static int record_host(gsv_ctx* c, record_dev dev, const uint8_t* in, const uint64_t* off, size_t n, size_t rec,
                       size_t res, uint8_t* out, uint8_t* status) {
    if (!c || (n && (!off || !out || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(in, off, n));
    std::vector<uint8_t> pad(n * rec);
    right_pad(in, off, n, rec, pad.data());
    Layout L;
    const RecordStage p(L, n, rec, res);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.in, pad.data()));
    GSVCHK(dev(c, s(p.in), n, s(p.out), s(p.st), c->stream));
    GSVCHK(s.out(out, p.out));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

int gsv_ecrecover_precompile_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out32,
                                   uint8_t* ok) {
    return record_host(c, gsv_ecrecover_precompile_batch_dev, in, off, n, 128, 32, out32, ok);
}

// ------------------------------------------------------------------ bn256Add / bn256ScalarMul (contracts.go:274-312)
// GSV_BN_G1_BITSERIAL=1 selects the bit-serial multiplication kernel (A/B timing and the tests only)
static int bn_g1_bitserial() {
    const char* e = getenv("GSV_BN_G1_BITSERIAL");
    return e && atoi(e) != 0;
}

int gsv_bn256_add_batch_dev(gsv_ctx* c, const uint8_t* d_in128, size_t n, uint8_t* d_out64, uint8_t* d_status,
                            void* stream) {
    if (!c || (n && (!d_in128 || !d_out64 || !d_status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BN_G1, st);
    return hip_err(gsv::launch_bn256_g1_add(d_in128, (uint32_t)n, d_out64, d_status, st));
}

int gsv_bn256_scalar_mul_batch_dev(gsv_ctx* c, const uint8_t* d_in96, size_t n, uint8_t* d_out64, uint8_t* d_status,
                                   void* stream) {
    if (!c || (n && (!d_in96 || !d_out64 || !d_status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BN_G1, st);
    return hip_err(gsv::launch_bn256_g1_mul(d_in96, (uint32_t)n, d_out64, d_status, bn_g1_bitserial(), st));
}

int gsv_bn256_add_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out64,
                        uint8_t* status) {
    return record_host(c, gsv_bn256_add_batch_dev, in, off, n, 128, 64, out64, status);
}

int gsv_bn256_scalar_mul_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out64,
                               uint8_t* status) {
    return record_host(c, gsv_bn256_scalar_mul_batch_dev, in, off, n, 96, 64, out64, status);
}

// ------------------------------------------------------------------ recoverPlain
int gsv_sender_batch(gsv_ctx* c, const uint8_t* sighash32, const uint8_t* r32, const uint8_t* s32,
                     const uint64_t* v, const uint8_t* v_big, size_t n, int homestead,
                     uint8_t* addr20_out, uint8_t* status) {
    if (!c || (n && (!sighash32 || !r32 || !s32 || !v || !v_big || !addr20_out || !status)) ||
        batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const SenderStage p(L, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.h, sighash32));
    GSVCHK(s.in(p.r, r32));
    GSVCHK(s.in(p.s, s32));
    GSVCHK(s.in(p.v, v));
    GSVCHK(s.in(p.vb, v_big));
    {
        KTimer t(c, GSV_K_ECRECOVER, c->stream);
        HIPCHK(gsv::launch_sender(s(p.h), s(p.r), s(p.s), s(p.v), s(p.vb), (uint32_t)n, homestead, c->gtab, s(p.a),
                                  s(p.st), c->stream));
    }
    GSVCHK(s.out(addr20_out, p.a));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

// ------------------------------------------------------------------ synthetic signer (bench data)
int gsv_synth_sign_dev(gsv_ctx* c, uint64_t seed, size_t n, uint8_t* d_msg32, uint8_t* d_sig65,
                       uint8_t* d_pub65, uint8_t* d_addr20, void* stream) {
    if (!c || (n && (!d_msg32 || !d_sig65)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    return hip_err(gsv::launch_synth_sign(seed, (uint32_t)n, c->gtab, d_msg32, d_sig65, d_pub65,
                                          d_addr20, st));
}

int gsv_synth_sign(gsv_ctx* c, uint64_t seed, size_t n, uint8_t* msg32, uint8_t* sig65,
                   uint8_t* pub65, uint8_t* addr20) {
    if (!c || (n && (!msg32 || !sig65)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    Layout L;
    const SynthSignStage p(L, n, pub65 != nullptr, addr20 != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    // s(p.pub), s(p.addr): nullptr when not asked for
    GSVCHK(gsv_synth_sign_dev(c, seed, n, s(p.msg), s(p.sig), s(p.pub), s(p.addr), c->stream));
    GSVCHK(s.out(msg32, p.msg));
    GSVCHK(s.out(sig65, p.sig));
    GSVCHK(s.out(pub65, p.pub));
    GSVCHK(s.out(addr20, p.addr));
    return s.finish();
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
    Staged s(c, L);
    if (s.rc) return s.rc;
    const SenderStage& q = p.snd;
    // one segment per decoding thread, back to back: they are p.pre's first pbytes bytes (poff[n])
    uint8_t* d_pre = s(p.pre);
    size_t w = 0;
    for (unsigned t = 0; t < nt; t++) {
        if (!tpre[t].empty())
            HIPCHK(hipMemcpyAsync(d_pre + w, tpre[t].data(), tpre[t].size(), hipMemcpyHostToDevice, c->stream));
        w += tpre[t].size();
    }
    GSVCHK(s.in(p.poff, poff.data()));
    GSVCHK(s.in(q.r, rr.data()));
    GSVCHK(s.in(q.s, ss.data()));
    GSVCHK(s.in(q.v, vv.data()));
    GSVCHK(s.in(q.vb, vb.data()));
    {
        KTimer t(c, GSV_K_SENDER_PREP, c->stream);
        HIPCHK(gsv::launch_keccak256(d_pre, s(p.poff), (uint32_t)n, s(q.h), c->stream));
    }
    {
        KTimer t(c, GSV_K_ECRECOVER, c->stream);
        HIPCHK(gsv::launch_sender(s(q.h), s(q.r), s(q.s), s(q.v), s(q.vb), (uint32_t)n, homestead, c->gtab, s(q.a),
                                  s(q.st), c->stream));
    }
    GSVCHK(s.out(addr_out, q.a));
    GSVCHK(s.out(status_out, q.st));
    GSVCHK(s.finish());
    for (size_t i = 0; i < n; i++)
        if (hst[i] != GSV_ST_OK) {
            status_out[i] = hst[i];
            memset(addr_out + i * 20, 0, 20);
        }
    return GSV_SUCCESS;
}

int gsv_tx_sender_batch(gsv_ctx* c, const uint8_t* rlp, const uint64_t* off, size_t n, const uint8_t* chain_id,
                        size_t chain_id_len, int signer_kind, uint8_t* addr20_out, uint8_t* status) {
    if (!c || (n && (!rlp || !off || !addr20_out || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (signer_kind < GSV_SIGNER_EIP155 || signer_kind > GSV_SIGNER_FRONTIER) return GSV_E_INVALID_ARG;
    if (chain_id_len && !chain_id) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(rlp, off, n));
    return tx_sender_impl(c, rlp, off, n, chain_id, chain_id_len, signer_kind, addr20_out, status);
}

}  // extern "C"

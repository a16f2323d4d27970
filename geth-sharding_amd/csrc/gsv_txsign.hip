// types.SignTx of the C ABI (gsv_ctx.h): the launch chain k_tx_sighash, k_ecsign, k_tx_seal (txsign.hip draws
// it) and the host form's staging.
#include "gsv_ctx.h"
#include "txsign_params.h"

using namespace gsv::api;

namespace {

// the checks gsv.h promises before any HIP call
bool signer_args_ok(const gsv_ctx* c, const uint8_t* chain_id, size_t chain_id_len, int signer_kind) {
    return c && chain_id_len <= gsv::txs::MAX_CHAIN_ID && !(chain_id_len && !chain_id) &&
           signer_kind >= GSV_SIGNER_EIP155 && signer_kind <= GSV_SIGNER_FRONTIER;
}

// bytes -> the kernels' word layout behind `lead` zero bytes (the arrays are zero already)
void pack_words(uint32_t* w, size_t lead, const uint8_t* b, size_t n) {
    for (size_t i = 0; i < n; i++) w[(lead + i) / 4] |= (uint32_t)b[i] << (8 * ((lead + i) % 4));
}

}  // namespace

extern "C" {

size_t gsv_tx_sign_work_bytes(size_t n) { return n * gsv::TXS_WORK_PER; }

int gsv_tx_sign_batch_dev(gsv_ctx* c, const uint8_t* d_rlp, const uint64_t* d_off, size_t n, const uint8_t* d_seckey32,
                          const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint8_t* d_out,
                          uint32_t* d_out_len, uint8_t* d_txhash32_out, uint8_t* d_status, uint8_t* d_work,
                          void* stream) {
    if (!signer_args_ok(c, chain_id, chain_id_len, signer_kind)) return GSV_E_INVALID_ARG;
    if ((n && (!d_rlp || !d_off || !d_seckey32 || !d_out || !d_out_len || !d_status || !d_work)) || batch_too_long(n) ||
        ((uintptr_t)d_work & 15) || ((uintptr_t)d_out_len & 3) || ((uintptr_t)d_txhash32_out & 3))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    const bool eip155 = signer_kind == GSV_SIGNER_EIP155;
    gsv::TxSignSuffix sfx = {};
    gsv::TxSignVTable vt = {};
    {
        uint8_t b[gsv::txs::MAX_SUFFIX > gsv::txs::MAX_V_ITEM ? gsv::txs::MAX_SUFFIX : gsv::txs::MAX_V_ITEM];
        sfx.len = (uint32_t)gsv::txs::suffix(chain_id, chain_id_len, eip155, b);
        pack_words(sfx.w, 4, b, sfx.len);  // behind one zero word (tx_flat.cuh TxStream)
        for (unsigned r = 0; r < 4; r++) {
            vt.len[r] = (uint32_t)gsv::txs::v_item(chain_id, chain_id_len, eip155, r, b);
            pack_words(vt.w + r * gsv::TXS_V_WORDS, 0, b, vt.len[r]);
        }
    }
    hipStream_t st = stream_of(c, stream);
    uint32_t* rec = (uint32_t*)d_work;
    uint8_t *msg = d_work + n * 16, *sig = d_work + n * 48, *sst = d_work + n * 113;
    {
        KTimer t(c, GSV_K_TX_SIGHASH, st);
        HIPCHK(gsv::launch_tx_sighash(d_rlp, d_off, (uint32_t)n, sfx, rec, (uint32_t*)msg, st));
    }
    {
        KTimer t(c, GSV_K_ECRECOVER, st);
        HIPCHK(gsv::launch_ecsign(msg, d_seckey32, (uint32_t)n, c->gtab, sig, sst, st));
    }
    KTimer t(c, GSV_K_TX_SEAL, st);
    return hip_err(gsv::launch_tx_seal(d_rlp, d_off, (uint32_t)n, vt, GSV_TX_SIGN_GROWTH(chain_id_len), rec, sig, sst,
                                       d_out, d_out_len, d_txhash32_out, d_status, st));
}

int gsv_tx_sign_batch(gsv_ctx* c, const uint8_t* rlp, const uint64_t* off, size_t n, const uint8_t* seckey32,
                      const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint8_t* out, uint32_t* out_len,
                      uint8_t* txhash32_out, uint8_t* status) {
    if (!signer_args_ok(c, chain_id, chain_id_len, signer_kind)) return GSV_E_INVALID_ARG;
    if ((n && (!off || !seckey32 || !out || !out_len || !status)) || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(rlp, off, n));  // the kernels trust off[i] <= off[i+1]
    const size_t bytes = off[n] - off[0], G = GSV_TX_SIGN_GROWTH(chain_id_len);
    const std::vector<uint64_t> rel = table_rebase(off, n);
    std::vector<uint8_t> slots(bytes + n * G);  // the staged slots; only each item's own bytes reach `out`
    Layout L;
    const TxSignStage p(L, n, gsv::TXS_WORK_PER, bytes, G, txhash32_out != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    s.secret(p.key);  // from here on the keys may be in HBM
    GSVCHK(s.in(p.key, seckey32));
    GSVCHK(s.in(p.rlp, rlp + off[0], bytes));
    GSVCHK(s.in(p.off, rel.data()));
    // s(p.hash): nullptr when not asked for
    GSVCHK(gsv_tx_sign_batch_dev(c, s(p.rlp), s(p.off), n, s(p.key), chain_id, chain_id_len, signer_kind, s(p.out),
                                 s(p.olen), s(p.hash), s(p.st), s(p.work), c->stream));
    GSVCHK(s.out(slots.data(), p.out));
    GSVCHK(s.out(out_len, p.olen));
    GSVCHK(s.out(txhash32_out, p.hash));
    GSVCHK(s.out(status, p.st));
    GSVCHK(s.finish());
    for (size_t i = 0; i < n; i++) {
        const size_t slot = rel[i] + i * G;
        // a length past the slot cannot come from the kernel; it is not trusted with the caller's memory
        if (out_len[i] > (rel[i + 1] - rel[i]) + G) return GSV_E_HIP;
        if (out_len[i]) memcpy(out + off[0] + slot, slots.data() + slot, out_len[i]);
    }
    return GSV_SUCCESS;
}

}  // extern "C"

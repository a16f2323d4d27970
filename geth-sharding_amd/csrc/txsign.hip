// Batched types.SignTx on gfx950 — the two kernels around the signature, one transaction per lane.
//
// Semantics restated from the reference:
//   core/types/transaction_signing.go:56-63  SignTx: h = s.Hash(tx); sig = crypto.Sign(h[:], prv);
//                                            tx.WithSignature(s, sig)
//   :155-165  EIP155Signer.Hash  = rlpHash([nonce, price, gas, to, value, data, chainId, 0, 0])
//   :207-216  FrontierSigner.Hash = rlpHash of the six fields (HomesteadSigner embeds it)
//   :141-151  EIP155Signer.SignatureValues: R, S the halves, V = sig[64] + 27, and with a chain id that
//             is not 0, V = sig[64] + 35 + 2 chainId
//   :195-203  FrontierSigner.SignatureValues (also Homestead's): V = sig[64] + 27
//   core/types/transaction.go:55-70  txdata: the nine-item list; :198-206 Hash() = rlpHash(tx)
//   rlp/encode.go writeBigInt: R, S and V without leading zero bytes
//
//   k_tx_sighash  decodes the flat item (tx_flat.cuh), classifies it, records where the six-item segment
//                 lies, and hashes header || segment || signer suffix: msg32 and a record per item.
//   (k_ecsign)    csrc/ecsign.hip, unchanged, over msg32 and the caller's keys: sig65 and a sign status.
//   k_tx_seal     merges the statuses, forms V || R || S, writes header || segment || V || R || S into the
//                 item's slot, hashes the same bytes (tx.Hash()), writes out_len.
// The chain id enters as kernel arguments the host prepared: the signer's suffix for the first kernel,
// the RLP items of V for recovery ids 0..3 for the second (V = recid + a per-call constant, up to 65
// bytes: no big-integer arithmetic is left for the device).  Both are copied to LDS once per block and
// read from there by lane-varying offsets.
#include "gsv_internal.h"
#include "tx_flat.cuh"

namespace gsv {

constexpr uint32_t TXS_MAX_ITEM = 1u << 20;  // gsv.h: a longer item is GSV_ST_BODY_TOO_LARGE

// block-uniform tail: the signer's suffix
struct SuffixTail {
    const uint32_t* w;
    GSV_DI uint32_t word(uint32_t k) const { return w[k]; }
};

__global__ __launch_bounds__(256) void k_tx_sighash(const uint8_t* __restrict__ rlp, const uint64_t* __restrict__ off,
                                                     uint32_t n, TxSignSuffix sfx, uint32_t* __restrict__ rec,
                                                     uint32_t* __restrict__ msg32) {
    __shared__ uint32_t s_sfx[TXS_SUFFIX_WORDS];
    if (threadIdx.x < TXS_SUFFIX_WORDS) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < TXS_SUFFIX_WORDS; j++) v = threadIdx.x == j ? sfx.w[j] : v;
        s_sfx[threadIdx.x] = v;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o0 = off[i], len64 = off[i + 1] - o0;
    uint32_t st = GSV_ST_BAD_RLP, seg_lo = 0, seg_len = 0, patch = TX_PATCH_NONE;
    uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (len64 > TXS_MAX_ITEM) st = GSV_ST_BODY_TOO_LARGE;
    else if (len64 > 0) {
        const uint32_t len = (uint32_t)len64;
        FlatView b(rlp + o0, len);
        if (flat_tx_decode(b, len, seg_lo, seg_len, patch)) {
            st = GSV_ST_OK;
            TxStream<SuffixTail> s{b, 0, 0, seg_lo, seg_len, patch, SuffixTail{s_sfx}, sfx.len};
            s.hdr = list_header_le(seg_len + sfx.len, s.hlen);
            uint64_t a[25];
            keccak_tx_stream(a, s);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                m[2 * j] = (uint32_t)a[j];
                m[2 * j + 1] = (uint32_t)(a[j] >> 32);
            }
        }
    }
    // the digest's bytes are the state words' little-endian bytes: msg32 as eight dwords (bad items sign
    // a zero message and are discarded by k_tx_seal)
    uint4* mo = (uint4*)(msg32 + (size_t)i * 8);
    mo[0] = make_uint4(m[0], m[1], m[2], m[3]);
    mo[1] = make_uint4(m[4], m[5], m[6], m[7]);
    ((uint4*)rec)[i] = make_uint4(seg_lo, seg_len, patch, st);
}

// per-lane tail V || R || S in LDS: word k of lane t at s_tail[k * 256 + t] (no bank conflicts)
constexpr uint32_t TXS_TAIL_WORDS = 36;  // one zero word, 133 bytes rounded up, one zero word
struct LaneTail {
    const uint32_t* col;  // s_tail + threadIdx.x
    GSV_DI uint32_t word(uint32_t k) const { return col[k * 256u]; }
};

GSV_DI void tail_put(uint32_t* s_tail, uint32_t pos, uint32_t byte) {
    ((uint8_t*)s_tail)[(((pos >> 2) + 1u) * 256u + threadIdx.x) * 4u + (pos & 3u)] = (uint8_t)byte;
}

// rlp of the big integer x[0..32) (big-endian) appended at tail position pos; returns the new position
GSV_DI uint32_t tail_put_u256(uint32_t* s_tail, uint32_t pos, const uint8_t x[32]) {
    uint32_t z = 0;
    bool lead = true;
#pragma unroll
    for (int j = 0; j < 32; j++) {
        lead = lead && x[j] == 0;
        z += lead ? 1u : 0u;
    }
    const uint32_t nb = 32u - z;
    if (!(nb == 1 && x[31] < 0x80)) tail_put(s_tail, pos++, 0x80u + nb);  // 0 is 0x80 alone
#pragma unroll
    for (int j = 0; j < 32; j++)
        if ((uint32_t)j >= z) tail_put(s_tail, pos + (uint32_t)j - z, x[j]);
    return pos + nb;
}

__global__ __launch_bounds__(256) void k_tx_seal(const uint8_t* __restrict__ rlp, const uint64_t* __restrict__ off,
                                                  uint32_t n, TxSignVTable vt, uint64_t growth,
                                                  const uint32_t* __restrict__ rec, const uint8_t* __restrict__ sig65,
                                                  const uint8_t* __restrict__ sign_st, uint8_t* __restrict__ out,
                                                  uint32_t* __restrict__ out_len, uint8_t* __restrict__ hash32,
                                                  uint8_t* __restrict__ status) {
    __shared__ uint32_t s_v[4 * TXS_V_WORDS];
    __shared__ uint32_t s_tail[TXS_TAIL_WORDS * 256];
    if (threadIdx.x < 4 * TXS_V_WORDS) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4 * TXS_V_WORDS; j++) v = threadIdx.x == j ? vt.w[j] : v;
        s_v[threadIdx.x] = v;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 r4 = ((const uint4*)rec)[i];
    const uint32_t st = r4.w != GSV_ST_OK ? r4.w : sign_st[i];  // the reference decodes before it signs
    status[i] = (uint8_t)st;
    if (st != GSV_ST_OK) {  // out_len 0, a zero hash, the slot untouched
        out_len[i] = 0;
        if (hash32)
            for (int j = 0; j < 32; j++) hash32[(size_t)i * 32 + j] = 0;
        return;
    }
    const uint8_t* sg = sig65 + (size_t)i * 65;
    uint8_t R[32], S[32];
#pragma unroll
    for (int j = 0; j < 32; j++) {
        R[j] = sg[j];
        S[j] = sg[32 + j];
    }
    const uint32_t recid = sg[64] & 3u;
    // tail = V item (the host's encoding for this recovery id, zero-padded words) || R || S
#pragma unroll
    for (uint32_t k = 0; k < TXS_TAIL_WORDS; k++)
        s_tail[k * 256u + threadIdx.x] = (k >= 1 && k <= TXS_V_WORDS) ? s_v[recid * TXS_V_WORDS + (k - 1)] : 0u;
    const uint32_t vlen = recid == 0 ? vt.len[0] : recid == 1 ? vt.len[1] : recid == 2 ? vt.len[2] : vt.len[3];
    uint32_t tl = tail_put_u256(s_tail, vlen, R);
    tl = tail_put_u256(s_tail, tl, S);

    const uint64_t o0 = off[i];
    const uint32_t len = (uint32_t)(off[i + 1] - o0);
    TxStream<LaneTail> s{FlatView(rlp + o0, len), 0, 0, r4.x, r4.y, r4.z, LaneTail{s_tail + threadIdx.x}, tl};
    s.hdr = list_header_le(r4.y + tl, s.hlen);
    const uint32_t L = s.total();  // <= len + growth (gsv.h GSV_TX_SIGN_GROWTH)
    // the slot: bytes up to the first aligned address, aligned dwords, the bytes left; nothing is written
    // outside [dst, dst + L)
    uint8_t* dst = out + o0 + (uint64_t)i * growth;
    uint32_t pos = 0;
    const uint32_t head = min((uint32_t)(-(uintptr_t)dst & 3u), L);
    if (head) {
        uint32_t w = s.dword(0);
        for (; pos < head; pos++) dst[pos] = (uint8_t)(w >> (8u * pos));
    }
    for (; pos + 4u <= L; pos += 4u) *(uint32_t*)(dst + pos) = s.dword(pos);
    if (pos < L) {
        uint32_t w = s.dword(pos);
        for (uint32_t j = 0; pos + j < L; j++) dst[pos + j] = (uint8_t)(w >> (8u * j));
    }
    out_len[i] = L;
    if (hash32) {  // tx.Hash(): Keccak-256 of the same bytes
        uint64_t a[25];
        keccak_tx_stream(a, s);
        uint8_t* h = hash32 + (size_t)i * 32;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            *(uint32_t*)(h + 8 * j) = (uint32_t)a[j];
            *(uint32_t*)(h + 8 * j + 4) = (uint32_t)(a[j] >> 32);
        }
    }
}

// ---------------------------------------------------------------------------- launchers
hipError_t launch_tx_sighash(const uint8_t* d_rlp, const uint64_t* d_off, uint32_t n, const TxSignSuffix& sfx,
                             uint32_t* d_rec, uint32_t* d_msg32, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tx_sighash, dim3((n + 255) / 256), dim3(256), 0, st, d_rlp, d_off, n, sfx, d_rec, d_msg32);
    return hipGetLastError();
}

hipError_t launch_tx_seal(const uint8_t* d_rlp, const uint64_t* d_off, uint32_t n, const TxSignVTable& vt,
                          uint64_t growth, const uint32_t* d_rec, const uint8_t* d_sig65, const uint8_t* d_sign_st,
                          uint8_t* d_out, uint32_t* d_out_len, uint8_t* d_hash32, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tx_seal, dim3((n + 255) / 256), dim3(256), 0, st, d_rlp, d_off, n, vt, growth, d_rec, d_sig65,
                       d_sign_st, d_out, d_out_len, d_hash32, d_status);
    return hipGetLastError();
}

}  // namespace gsv

// What types.SignTx's kernels need of the signer and the chain id, as bytes: plain C++17, free of HIP
// (tests/native/tx_sign_params_host.cpp compiles it with g++).  csrc/gsv_txsign.hip packs the results into
// the kernels' arguments (gsv_internal.h TxSignSuffix, TxSignVTable).
//   core/types/transaction_signing.go:155-165  EIP155Signer.Hash appends chainId, uint(0), uint(0)
//   :141-151  EIP155Signer.SignatureValues: V = sig[64] + 27, and V += 2 chainId + 8 when chainId != 0
//   :195-203  FrontierSigner.SignatureValues: V = sig[64] + 27
//   rlp/encode.go writeBigInt / writeUint: 0 is 0x80, a value below 128 its own byte
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace gsv {
namespace txs {

constexpr size_t MAX_CHAIN_ID = 64;              // bytes, as gsv_notary_prepare
constexpr size_t MAX_SUFFIX = 2 + MAX_CHAIN_ID + 2;  // b8 40 || 64 bytes || 80 80
constexpr size_t MAX_V_ITEM = 2 + MAX_CHAIN_ID + 1;  // b8 41 || 65 bytes

// rlp of the big-endian unsigned integer d[0 .. n) (leading zero bytes allowed), n <= 65; returns its length
inline size_t put_bigint(uint8_t* o, const uint8_t* d, size_t n) {
    while (n && d[0] == 0) {
        d++;
        n--;
    }
    if (n == 0) {
        o[0] = 0x80;
        return 1;
    }
    if (n == 1 && d[0] < 0x80) {
        o[0] = d[0];
        return 1;
    }
    size_t h = 1;
    if (n < 56) o[0] = (uint8_t)(0x80 + n);
    else {
        o[0] = 0xb8;
        o[1] = (uint8_t)n;
        h = 2;
    }
    memcpy(o + h, d, n);
    return h + n;
}

// what the signer's Hash appends to the six fields; out holds MAX_SUFFIX bytes; returns the length
inline size_t suffix(const uint8_t* cid, size_t cidlen, bool eip155, uint8_t* out) {
    if (!eip155) return 0;
    size_t w = put_bigint(out, cid, cidlen);
    out[w++] = 0x80;
    out[w++] = 0x80;
    return w;
}

// the RLP item of V for recovery id `recid` (0..3); out holds MAX_V_ITEM bytes; returns the length
inline size_t v_item(const uint8_t* cid, size_t cidlen, bool eip155, unsigned recid, uint8_t* out) {
    uint8_t v[MAX_CHAIN_ID + 1] = {0};  // big-endian
    bool zero = true;
    for (size_t i = 0; i < cidlen; i++) zero = zero && cid[i] == 0;
    unsigned add = recid + 27;
    if (eip155 && !zero) {
        memcpy(v + sizeof(v) - cidlen, cid, cidlen);
        unsigned carry = 0;  // v = 2 chainId
        for (size_t i = sizeof(v); i-- > 0;) {
            unsigned d = 2u * v[i] + carry;
            v[i] = (uint8_t)d;
            carry = d >> 8;
        }
        add = recid + 35;
    }
    for (size_t i = sizeof(v); i-- > 0 && add;) {  // v += add
        unsigned d = v[i] + add;
        v[i] = (uint8_t)d;
        add = d >> 8;
    }
    return put_bigint(out, v, sizeof(v));
}

}  // namespace txs
}  // namespace gsv

// Packing of variable-length public keys into the device layout of gsv_ecdsa_verify_batch_dev and
// gsv_pubkey_parse_batch_dev, free of HIP (plain C++17; tests/native/pubkey_pack_host.cpp compiles it
// with g++).  Key i = pub[off[i] .. off[i+1]) becomes row i of rows65 (65 bytes, zero-padded) and one
// length byte: 33 or 65, and 0 for every other length (no such key parses: eckey_pubkey_parse accepts
// 33 and 65 bytes only), whose row stays zero.  The caller has checked off[i] <= off[i+1].
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace gsv {

inline void pubkey_pack(const uint8_t* pub, const uint64_t* off, size_t n, uint8_t* rows65, uint8_t* len) {
    for (size_t i = 0; i < n; i++) {
        const uint64_t l = off[i + 1] - off[i];
        const size_t keep = (l == 33 || l == 65) ? (size_t)l : 0;
        uint8_t* row = rows65 + i * 65;
        if (keep) memcpy(row, pub + off[i], keep);
        memset(row + keep, 0, 65 - keep);
        len[i] = (uint8_t)keep;
    }
}

}  // namespace gsv

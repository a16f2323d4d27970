// Host build of csrc/txsign_params.h (the signer's suffix and the RLP items of V that gsv_tx_sign_batch
// prepares for its kernels) for tests/test_tx_sign_cpu.py.
#include "../../geth-sharding_amd/csrc/txsign_params.h"

extern "C" {

int txs_suffix(const uint8_t* cid, int cidlen, int eip155, uint8_t* out) {
    return (int)gsv::txs::suffix(cid, (size_t)cidlen, eip155 != 0, out);
}

int txs_v_item(const uint8_t* cid, int cidlen, int eip155, int recid, uint8_t* out) {
    return (int)gsv::txs::v_item(cid, (size_t)cidlen, eip155 != 0, (unsigned)recid, out);
}

}  // extern "C"

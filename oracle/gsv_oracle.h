/*
 * TEST INFRASTRUCTURE ONLY — the CPU oracle for the collation-validation hot path.
 *
 * A plain-C restatement of the reference algorithms, written for clarity, used
 * only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the
 * checker.  Never linked into, loaded by, or called from the product library
 * (geth-sharding_amd/csrc -> libgsv.so).  Each function cites the reference
 * file:line it restates.  Pinned against the reference's golden vectors and
 * against the reference's own C code (oracle/_ref) in tests/test_oracle.py.
 */
#ifndef GSV_ORACLE_H
#define GSV_ORACLE_H
#include <stddef.h>
#include <stdint.h>

/* status codes: identical values to include/gsv.h */
enum {
    OR_OK = 0,
    OR_INVALID_MSG_LEN = 1,
    OR_INVALID_SIG_LEN = 2,
    OR_INVALID_RECID = 3,
    OR_RECOVER_FAILED = 4,
    OR_INVALID_SIG = 5,
    OR_INVALID_CHAIN_ID = 6,
    OR_INVALID_PUBKEY = 7,
    OR_BAD_RLP = 8,
    OR_BN_BAD_INPUT = 9,
};
/* oracle_secp_chain_check results below -1 (-1 = the chain holds, >= 0 = first failing index) */
enum { OR_CHAIN_DEGENERATE = -2, OR_CHAIN_BAD_BASE = -3 };

void oracle_keccak256(const uint8_t *in, size_t len, uint8_t out[32]);
void oracle_keccak256_batch(const uint8_t *data, const uint64_t *off, long n, uint8_t *out32);
void oracle_keccakf1600(uint64_t st[25]);
void oracle_keccak_sponge(const uint8_t *in, size_t len, int rate, uint8_t dsbyte, uint8_t *out,
                          size_t outlen);

int oracle_ecrecover(uint8_t pub65[65], const uint8_t sig65[65], const uint8_t msg32[32]);
void oracle_ecrecover_batch(const uint8_t *msg32, const uint8_t *sig65, long n, uint8_t *pub65,
                            uint8_t *status, int threads);
/* first i with Q[i] != Q[i-1] + B or Q[i] no curve point (n affine points X || Y, big-endian), -1 if
 * none; no inversions (cross-multiplied chord equations) */
long oracle_secp_chain_check(const uint8_t *q64, long n, const uint8_t base64[64], int threads);
int oracle_recover_plain(uint8_t addr20[20], const uint8_t sighash[32], const uint8_t *r, size_t rlen,
                         const uint8_t *s, size_t slen, const uint8_t *v, size_t vlen, int homestead);
int oracle_tx_sender(uint8_t addr20[20], const uint8_t *rlp, size_t len, const uint8_t *chain_id,
                     size_t chain_id_len, int signer_kind);
/* Sender's Keccak / recovery provider: NULL = this restatement; the CPU baseline passes the
 * reference's own (oracle/_ref gsvref_keccak256 / gsvref_ecrecover) */
typedef int (*or_keccak_fn)(uint8_t *out32, const uint8_t *in, size_t len);
typedef int (*or_recover_fn)(uint8_t *pub65, const uint8_t *sig65, const uint8_t *msg32);
void oracle_set_crypto(or_keccak_fn k, or_recover_fn r);
void oracle_tx_sender_many(const uint8_t *rlp, const uint64_t *off, long n, const uint8_t *cid, size_t cidlen,
                           int signer_kind, uint8_t *addr20, uint8_t *status, int threads);
int oracle_tx_sighash(uint8_t out32[32], const uint8_t *rlp, size_t len, const uint8_t *chain_id,
                      size_t chain_id_len, int signer_kind);

void oracle_derive_sha_bytes(const uint8_t *body, size_t n, uint8_t root[32]);
int oracle_trie_root(const uint8_t *keys, const uint64_t *koff, const uint8_t *vals,
                     const uint64_t *voff, long n, uint8_t root[32]);
long oracle_blob_serialize(const uint8_t *data, const uint64_t *off, const uint8_t *skip_evm, long n,
                           uint8_t *out, long cap);
long oracle_blob_deserialize(const uint8_t *data, size_t len, uint8_t *out, uint64_t *off,
                             uint8_t *skip_evm, long max_blobs);

int oracle_secp_pubkey(uint8_t pub65[65], const uint8_t seckey[32]);
void oracle_synth_sign_many(uint64_t seed, long n, uint8_t *msg32, uint8_t *sig65, int threads);
int oracle_secp_sign(uint8_t sig65[65], const uint8_t msg32[32], const uint8_t seckey[32],
                     const uint8_t nonce32[32]);

/* bn256_oracle.c: 1 true / 0 false / -1 error (core/vm/contracts.go:333-360) */
int oracle_bn256_pairing_check(const uint8_t *in, size_t len);
int oracle_bn256_miller(const uint8_t in192[192], uint8_t out384[384]);
int oracle_bn256_final_exp(const uint8_t in384[384], uint8_t out384[384]);
int oracle_bn256_g1_mul(uint8_t out64[64], const uint8_t *in64, const uint8_t k32[32]);
int oracle_bn256_g2_mul(uint8_t out128[128], const uint8_t *in128, const uint8_t k32[32]);
int oracle_bn256_g2_check(const uint8_t in128[128]);
uint64_t oracle_bn256_fp_mul_count(int reset);
#endif

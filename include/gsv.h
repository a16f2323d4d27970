/*
 * gsv.h — C ABI of the MI355X-native batch validation engine for geth-sharding's
 * collation-validation hot path (libgsv.so, HIP for gfx950).
 *
 * Plain C linkage, plain pointers and sizes, no torch / HIP types in the signatures, so
 * the reference's Go side can bind it with a cgo preamble exactly as it binds
 * crypto/secp256k1/ext.h today (see INTEGRATION.md for the stub).
 *
 * Every entry point replaces a per-item reference call with a batch:
 *   gsv_ecrecover_batch        <- secp256k1_ext_ecdsa_recover (crypto/secp256k1/ext.h:30-47)
 *                                 via secp256k1.RecoverPubkey (crypto/secp256k1/secp256.go:105-122)
 *                                 / crypto.Ecrecover (crypto/signature_cgo.go:31)
 *   gsv_ecdsa_verify_batch     <- secp256k1_ext_ecdsa_verify (crypto/secp256k1/ext.h) via
 *                                 secp256k1.VerifySignature (crypto/secp256k1/secp256.go:124-134)
 *                                 / crypto.VerifySignature (crypto/signature_cgo.go:63-68)
 *   gsv_pubkey_parse_batch     <- secp256k1_ext_reencode_pubkey (crypto/secp256k1/ext.h) via
 *                                 DecompressPubkey / CompressPubkey (secp256.go:136-169)
 *   gsv_ecdsa_sign_batch       <- secp256k1_ecdsa_sign_recoverable with secp256k1_nonce_function_rfc6979
 *                                 via secp256k1.Sign (crypto/secp256k1/secp256.go:70-99) / crypto.Sign
 *                                 (crypto/signature_cgo.go:54-61)
 *   gsv_pubkey_create_batch    <- secp256k1_ec_pubkey_create (libsecp256k1/src/secp256k1.c), the key
 *                                 derivation behind crypto.ToECDSA / crypto.PubkeyToAddress
 *   gsv_secp256k1_scalar_mul_batch <- secp256k1_ext_scalar_mul (crypto/secp256k1/ext.h:104-142) via
 *                                 BitCurve.ScalarMult / ScalarBaseMult (crypto/secp256k1/curve.go:221-259)
 *   gsv_ecdh_batch             <- ecies.PrivateKey.GenerateShared (crypto/ecies/ecies.go:121-138) and the
 *                                 key derivation of ecies.Encrypt / Decrypt (ecies.go:264-277, 347-356);
 *                                 the RLPx handshake's two GenerateShared calls (p2p/rlpx.go:243, 276)
 *   gsv_ecies_decrypt_batch / gsv_ecies_encrypt_batch <- ecies.PrivateKey.Decrypt / ecies.Encrypt
 *                                 (crypto/ecies/ecies.go:246-366): the RLPx handshake packets
 *                                 (p2p/rlpx.go:434-511), whisper's asymmetric envelopes
 *   gsv_sender_batch           <- recoverPlain (core/types/transaction_signing.go:222-247)
 *                                 + crypto.ValidateSignatureValues (crypto/crypto.go:181-192)
 *   gsv_tx_sender_batch        <- types.Sender(signer, tx) (core/types/transaction_signing.go:72-89,
 *                                 127-137, 182-184, 218-220) over RLP-encoded txs
 *   gsv_tx_sign_batch          <- types.SignTx(tx, signer, prv) (core/types/transaction_signing.go:56-63):
 *                                 signer.Hash, crypto.Sign, tx.WithSignature (SignatureValues :141-151,
 *                                 195-203) and tx.Hash() over RLP-encoded txs; behind keystore.SignTx
 *   gsv_keccak256_batch        <- crypto.Keccak256 (crypto/crypto.go:43-49; crypto/sha3/hashes.go:16)
 *   gsv_chunk_root_batch       <- Collation.CalculateChunkRoot (sharding/collation.go:115-119)
 *                                 = types.DeriveSha(Chunks(body)) (core/types/derive_sha.go:32-41)
 *   gsv_bn256_pairing_check_batch <- bn256.PairingCheck (crypto/bn256/cloudflare/bn256.go:313-327)
 *                                 as driven by the bn256Pairing precompile (core/vm/contracts.go:333-360)
 *   gsv_notary_validate_shards <- the notary's per-collation validation (sharding/notary/notary.go:413-496
 *                                 + sharding/collation.go:193-206 DeserializeBlobToTx + Sender)
 *   gsv_derive_sha_batch       <- types.DeriveSha(list) (core/types/derive_sha.go:32-41) for any
 *                                 DerivableList: tx root (core/block_validator.go:70), receipt root (:92)
 *   gsv_collation_poc_batch    <- Collation.CalculatePOC(salt) (sharding/collation.go:124-136)
 *   gsv_collation_header_verify_batch <- CollationHeader.Hash (sharding/collation.go:66-71) and the
 *                                 proposer signature made by SMCClient.Sign (sharding/mainchain/
 *                                 smc_client.go:245-248, signed at sharding/proposer/proposer.go:83)
 *   gsv_blob_serialize_batch   <- utils.Serialize (sharding/utils/marshal.go:71-123), behind
 *                                 sharding.SerializeTxToBlob (sharding/collation.go:158-174)
 *   gsv_blob_deserialize_batch <- utils.Deserialize (sharding/utils/marshal.go:144-198), behind
 *                                 sharding.DeserializeBlobToTx (sharding/collation.go:193-206)
 *   gsv_proposer_create_collations <- proposer.createCollation (sharding/proposer/proposer.go:55-92):
 *                                 SerializeTxToBlob, CalculateChunkRoot, Hash(), SMCClient.Sign
 *
 *   gsv_ecrecover_precompile_batch <- the ecrecover precompile's Run (core/vm/contracts.go:78-101)
 *   gsv_bn256_add_batch        <- the bn256Add precompile's Run (core/vm/contracts.go:274-289)
 *                                 = G1.Unmarshal x 2, G1.Add, G1.Marshal (crypto/bn256/cloudflare/bn256.go:62-67)
 *   gsv_bn256_scalar_mul_batch <- the bn256ScalarMul precompile's Run (core/vm/contracts.go:297-312)
 *                                 = G1.Unmarshal, G1.ScalarMult, G1.Marshal (bn256.go:70-78)
 *   gsv_modexp_batch           <- the bigModExp precompile's Run (core/vm/contracts.go:226-252, EIP-198)
 *                                 = big.Int.Exp(base, exp, mod) over operands of caller-chosen length
 *   gsv_sha256_batch           <- the sha256hash precompile's Run (core/vm/contracts.go:114-117)
 *                                 = crypto/sha256.Sum256
 *   gsv_ripemd160_batch        <- the ripemd160hash precompile's Run (core/vm/contracts.go:129-133)
 *                                 = common.LeftPadBytes(ripemd160.New().Write(input).Sum(nil), 32)
 *                                 (vendor/golang.org/x/crypto/ripemd160)
 *   gsv_block_header_hash_batch <- Header.Hash() and Header.HashNoNonce() (core/types/block.go:99-122) over
 *                                 RLP-encoded headers
 *   gsv_calc_difficulty_batch  <- ethash.CalcDifficulty (consensus/ethash/consensus.go:297-459)
 *   gsv_ethash_verify_headers_batch <- Ethash.VerifyHeaders (consensus/ethash/consensus.go:90-166): verifyHeaderWorker
 *                                 and verifyHeader (:223-285) with uncle = false, VerifySeal included
 *   gsv_bloom9_batch           <- bloom9 (core/types/bloom9.go:115-127), behind BloomLookup (:131-136)
 *   gsv_receipts_verify_batch  <- types.CreateBloom (bloom9.go:94-113), the receipt root and the three receipt
 *                                 compares of BlockValidator.ValidateState (core/block_validator.go:80-95) over
 *                                 RLP-encoded receipts (core/types/receipt.go:67-128)
 *   gsv_bloombits_generate_batch <- bloombits.Generator (core/bloombits/generator.go:52-87) over whole sections,
 *                                 as BloomIndexer.Process / Commit feed it (eth/bloombits.go:126-141)
 *   gsv_bitset_compress_batch  <- bitutil.CompressBytes / DecompressBytes (common/bitutil/compress.go:60-170)
 *   gsv_bloombits_match_batch  <- bloombits.NewMatcher and what a Matcher session computes
 *                                 (core/bloombits/matcher.go:92-131, :182-211, :337-366)
 *   gsv_bloom_filter_batch     <- bloomFilter (eth/filters/filter.go:278-305) after filters.New's flattening (:62-93)
 *   gsv_clique_fold            <- the snapshot half of Clique.VerifyHeaders on the host: verifyCascadingFields'
 *                                 checkpoint compare, verifySeal and Snapshot.apply over records of recovered signers
 *                                 (consensus/clique/clique.go:351-367, :478-502, consensus/clique/snapshot.go:175-285)
 *
 * Conventions
 *   - Return value: GSV_SUCCESS (0) or a negative GSV_E_* API/HIP error. A bad ITEM never fails
 *     the batch: it gets a per-item status code (GSV_ST_*) mirroring the reference's errors.
 *   - Host-pointer entry points copy inputs to HBM, run, and copy results back (synchronous).
 *   - *_dev entry points take DEVICE pointers already resident in HBM and a hipStream_t passed
 *     as void*; they only enqueue: they never allocate device memory and never synchronize, so a
 *     *_dev call can be captured into a HIP graph (hipStreamBeginCapture).
 *   - *_dev entry points whose launch depends on host-side arguments (offset tables, chain id,
 *     salt, batch size: chunk root, pairing, notary, DeriveSha, POC, headers) need that exact
 *     argument set PREPARED first by the matching gsv_*_prepare call, which builds the trie plans
 *     and lane tables, uploads them to HBM and sizes the workspace (it may allocate and
 *     synchronize).  Unprepared -> GSV_E_NOT_PREPARED, nothing enqueued.  A context keeps its 32
 *     most recently used prepared shapes (<= 32 GiB); a HIP graph captured from a shape must not
 *     be replayed after that shape was dropped, and the caller orders graph replays against other
 *     uses of the same shape (non-captured calls on different streams are ordered by the library).
 *   - One gsv_ctx per device; a context is safe to use from several threads on distinct streams
 *     for the *_dev calls; host-pointer calls serialize on the context's internal stream.
 *   - stream = NULL selects the context stream, a blocking stream: it is ordered both ways with work
 *     on the process's legacy default (NULL) stream, such as PyTorch's default stream.  Work on other
 *     non-blocking streams is the caller's to order (events), as for any stream argument.  Capture
 *     HIP graphs on an explicit stream (a NULL-stream capture would join that implicit ordering).
 */
#ifndef GSV_H
#define GSV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSV_ABI_VERSION 2 /* 2: streams owned by the context (gsv_stream_create) */

/* ---- API / HIP errors (return values) ---- */
#define GSV_SUCCESS 0
#define GSV_E_INVALID_ARG (-1)
#define GSV_E_HIP (-2)
#define GSV_E_NOMEM (-3)
#define GSV_E_NO_DEVICE (-4)
#define GSV_E_TOO_LARGE (-5) /* e.g. collation body > 2^20 (sharding/collation.go:45) */
#define GSV_E_RCCL (-6)
#define GSV_E_NOT_PREPARED (-7) /* *_dev call whose host-side arguments were not gsv_*_prepare'd */

/* ---- per-item status codes (mirror the reference's error values) ---- */
#define GSV_ST_OK 0
#define GSV_ST_INVALID_MSG_LEN 1   /* secp256k1.ErrInvalidMsgLen       secp256.go:55 */
#define GSV_ST_INVALID_SIG_LEN 2   /* secp256k1.ErrInvalidSignatureLen secp256.go:56 */
#define GSV_ST_INVALID_RECID 3     /* secp256k1.ErrInvalidRecoveryID   secp256.go:57 */
#define GSV_ST_RECOVER_FAILED 4    /* secp256k1.ErrRecoverFailed       secp256.go:61 */
#define GSV_ST_INVALID_SIG 5       /* types.ErrInvalidSig              transaction.go:35 */
#define GSV_ST_INVALID_CHAIN_ID 6  /* types.ErrInvalidChainId          transaction_signing.go */
#define GSV_ST_INVALID_PUBKEY 7    /* "invalid public key"             transaction_signing.go:240 */
#define GSV_ST_BAD_RLP 8           /* rlp decode error of the tx */
#define GSV_ST_BN_BAD_INPUT 9      /* bn256 unmarshal / curve / subgroup failure */
#define GSV_ST_PROPOSER_MISMATCH 10 /* recovered signer != header ProposerAddress */
#define GSV_ST_INVALID_KEY 11      /* secp256k1.ErrInvalidKey          secp256.go:58 */
#define GSV_ST_INVALID_CURVE 12    /* ecies.ErrInvalidCurve            ecies/ecies.go:47 */
#define GSV_ST_BODY_TOO_LARGE 13   /* SerializeTxToBlob's size error   sharding/collation.go:169-171 */
#define GSV_ST_INVALID_MESSAGE 14  /* ecies.ErrInvalidMessage          ecies/ecies.go:143 */
#define GSV_ST_MODEXP_TOO_LONG 15  /* a modexp length above GSV_MODEXP_MAX_LEN: not the reference's, see there */
#define GSV_ST_INVALID_DIFFICULTY 16 /* ethash errInvalidDifficulty    consensus/ethash/consensus.go:56 */
#define GSV_ST_INVALID_MIX_DIGEST 17 /* ethash errInvalidMixDigest     consensus/ethash/consensus.go:57 */
#define GSV_ST_INVALID_POW 18        /* ethash errInvalidPoW           consensus/ethash/consensus.go:58 */
#define GSV_ST_NONCE_NOT_FOUND 19    /* the sealer gave up after max_attempts nonces: not the reference's, whose
                                        mine() runs until it is aborted (consensus/ethash/sealer.go:110-118) */
/* block headers (gsv_ethash_verify_headers_batch), in the order verifyHeaderWorker and verifyHeader test them */
#define GSV_ST_HEADER_TOO_WIDE 20    /* a header that decodes, with Difficulty or Time above 32 bytes or Number above
                                        8: not the reference's, whose big.Int fields have no bound */
#define GSV_ST_UNKNOWN_ANCESTOR 21   /* consensus.ErrUnknownAncestor   consensus/errors.go:24, consensus.go:159-161 */
#define GSV_ST_EXTRA_TOO_LONG 22     /* "extra-data too long"          consensus/ethash/consensus.go:225-227 */
#define GSV_ST_FUTURE_BLOCK 23       /* consensus.ErrFutureBlock       consensus/errors.go:32, consensus.go:234-236 */
#define GSV_ST_ZERO_BLOCK_TIME 24    /* ethash errZeroBlockTime        consensus.go:51, :238-240 */
#define GSV_ST_WRONG_DIFFICULTY 25   /* "invalid difficulty"           consensus.go:242-246 */
#define GSV_ST_GAS_LIMIT_CAP 26      /* "invalid gasLimit"             consensus.go:248-251 */
#define GSV_ST_GAS_USED 27           /* "invalid gasUsed"              consensus.go:253-255 */
#define GSV_ST_GAS_LIMIT_BOUNDS 28   /* "invalid gas limit"            consensus.go:258-266 */
#define GSV_ST_INVALID_NUMBER 29     /* consensus.ErrInvalidNumber     consensus/errors.go:36, consensus.go:268-270 */
#define GSV_ST_BAD_PRO_DAO_EXTRA 30  /* misc.ErrBadProDAOExtra         consensus/misc/dao.go:32, :58-61 */
#define GSV_ST_BAD_NO_DAO_EXTRA 31   /* misc.ErrBadNoDAOExtra          consensus/misc/dao.go:36, :62-66 */
#define GSV_ST_FORK_HASH 32          /* "homestead gas reprice fork"   consensus/misc/forks.go:36-39 */
/* receipts (gsv_receipts_verify_batch), in the order the receipt half of ValidateState tests them */
#define GSV_ST_RECEIPT_STATUS 33       /* "invalid receipt status"     core/types/receipt.go:116-128 */
#define GSV_ST_GAS_USED_MISMATCH 34    /* "invalid gas used"           core/block_validator.go:82-84 */
#define GSV_ST_INVALID_BLOOM 35        /* "invalid bloom"              core/block_validator.go:87-90 */
#define GSV_ST_INVALID_RECEIPT_ROOT 36 /* "invalid receipt root hash"  core/block_validator.go:92-95 */
/* bitset decompression (gsv_bitset_decompress_batch): common/bitutil/compress.go:21-37 */
#define GSV_ST_BITSET_MISSING_DATA 37      /* errMissingData       "missing bytes on input"      :24 */
#define GSV_ST_BITSET_UNREFERENCED_DATA 38 /* errUnreferencedData  "extra bytes on input"        :28 */
#define GSV_ST_BITSET_EXCEEDED_TARGET 39   /* errExceededTarget    "target data size exceeded"   :32 */
#define GSV_ST_BITSET_ZERO_CONTENT 40      /* errZeroContent       "zero byte in input content"  :36 */
/* clique (gsv_clique_fold and the records it reads), in the order verifyHeader tests them: consensus/clique/clique.go */
#define GSV_ST_CLIQUE_CHECKPOINT_BENEFICIARY 41 /* errInvalidCheckpointBeneficiary  :81, :280-282 */
#define GSV_ST_CLIQUE_INVALID_VOTE 42           /* errInvalidVote                   :85, :284-286, snapshot.go:236-238 */
#define GSV_ST_CLIQUE_CHECKPOINT_VOTE 43        /* errInvalidCheckpointVote         :89, :287-289 */
#define GSV_ST_CLIQUE_MISSING_VANITY 44         /* errMissingVanity                 :93, :291-293 */
#define GSV_ST_CLIQUE_MISSING_SIGNATURE 45      /* errMissingSignature              :97, :294-296, :178-180 */
#define GSV_ST_CLIQUE_EXTRA_SIGNERS 46          /* errExtraSigners                  :101, :299-301 */
#define GSV_ST_CLIQUE_CHECKPOINT_SIGNERS 47     /* errInvalidCheckpointSigners      :106, :302-304, :356-365 */
#define GSV_ST_CLIQUE_MIX_DIGEST 48             /* errInvalidMixDigest              :109, :306-308 */
#define GSV_ST_CLIQUE_UNCLE_HASH 49             /* errInvalidUncleHash              :112, :310-312 */
#define GSV_ST_CLIQUE_DIFFICULTY 50             /* errInvalidDifficulty             :116, :314-318, :494-501 */
#define GSV_ST_CLIQUE_INVALID_TIMESTAMP 51      /* ErrInvalidTimestamp              :120, :347-349 */
#define GSV_ST_CLIQUE_UNAUTHORIZED 52           /* errUnauthorized                  :127, :483-493, snapshot.go:208-215 */
#define GSV_ST_CLIQUE_VOTING_CHAIN 53           /* errInvalidVotingChain            :124, snapshot.go:181-188 */

/* signer kinds for gsv_tx_sender_batch and gsv_tx_sign_batch (core/types/transaction_signing.go) */
#define GSV_SIGNER_EIP155 0
#define GSV_SIGNER_HOMESTEAD 1
#define GSV_SIGNER_FRONTIER 2

/* pairing verdicts (core/vm/contracts.go:333-360: true32 / false32 / errBadPairingInput) */
#define GSV_PAIRING_FALSE 0
#define GSV_PAIRING_TRUE 1
#define GSV_PAIRING_BAD_INPUT 2

typedef struct gsv_ctx gsv_ctx;

/* ---- context ---- */
int gsv_device_count(void);
/* Creates a context on HIP device `device`; builds the device-resident precomputed tables
 * (secp256k1 fixed-base comb, Keccak round constants). ~once per process, like the reference's
 * global secp256k1 context (crypto/secp256k1/secp256.go:45-52). */
int gsv_ctx_create(int device, gsv_ctx **out);
void gsv_ctx_destroy(gsv_ctx *ctx);
const char *gsv_error_string(int err);
int gsv_abi_version(void);

/* Kernel timing (HIP events around each launch on the launching stream; off by default). */
int gsv_ctx_set_timing(gsv_ctx *ctx, int enable);
/* kernel ids for gsv_ctx_kernel_time */
#define GSV_K_KECCAK 0
#define GSV_K_ECRECOVER 1
#define GSV_K_CHUNK_LEAF 2
#define GSV_K_CHUNK_LEVEL 3
#define GSV_K_PAIRING 4
#define GSV_K_SENDER_PREP 5
#define GSV_K_BN_PREPARE 6 /* pair decode + G1 curve + G2 subgroup checks */
#define GSV_K_BN_FINAL 7   /* per-check product + final exponentiation */
#define GSV_K_NOTARY 8     /* blob index + per-tx decode/sighash/recover of the notary path */
#define GSV_K_DERIVE_LEAF 9 /* generic DeriveSha leaf encode + hash */
#define GSV_K_HEADER 10    /* collation header hashing + signer comparison */
#define GSV_K_BN_G1 11     /* bn256Add / bn256ScalarMul: one launch per call */
#define GSV_K_COUNT 12     /* the ids above */
/* Ids added behind GSV_K_COUNT (its value is part of ABI 2); gsv_ctx_kernel_time takes every id below
 * GSV_K_END. */
#define GSV_K_ECIES 12     /* the message half of ECIES: tag + AES-128-CTR, one launch per call */
#define GSV_K_END 13
/* Ids added behind GSV_K_END (its value, too, is pinned as part of ABI 2); gsv_ctx_kernel_time takes every
 * id below GSV_K_LIMIT. */
#define GSV_K_TX_SIGHASH 13 /* types.SignTx: decode + sighash of gsv_tx_sign_batch, one launch per call */
#define GSV_K_TX_SEAL 14    /* types.SignTx: V, R, S, the signed encoding and tx.Hash(), one launch per call */
#define GSV_K_LIMIT 15
/* Ids added behind GSV_K_LIMIT (pinned like the two before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_BOUND. */
#define GSV_K_MODEXP 15     /* the modexp precompile: one launch per call of the device form */
#define GSV_K_BOUND 16
/* Ids added behind GSV_K_BOUND (pinned like the three before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_CAP. */
#define GSV_K_SHA256 16     /* the sha256hash precompile: one launch per call */
#define GSV_K_RIPEMD160 17  /* the ripemd160hash precompile: one launch per call */
#define GSV_K_CAP 18
/* Ids added behind GSV_K_CAP (pinned like the four before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_TOP. */
#define GSV_K_ETHASH_ITEMS 18 /* ethash dataset items: one launch per call */
#define GSV_K_ETHASH_LIGHT 19 /* ethash hashimotoLight / VerifySeal: one launch per call */
#define GSV_K_TOP 20
/* Ids added behind GSV_K_TOP (pinned like the five before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_PEAK. */
#define GSV_K_ETHASH_FULL 20   /* ethash hashimotoFull / VerifySeal over the dataset: one launch per call */
#define GSV_K_ETHASH_SEARCH 21 /* ethash nonce search: one launch per gsv_ethash_search_dev */
#define GSV_K_ETHASH_FINISH 22 /* the search's finish launch (the winners' rows): one per gsv_ethash_search_dev */
#define GSV_K_PEAK 23
/* Ids added behind GSV_K_PEAK (pinned like the six before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_SUMMIT. */
#define GSV_K_BLOCK_HEADER 23 /* types.Header decode + Hash / HashNoNonce: one launch per call */
#define GSV_K_BLOCK_RULES 24  /* verifyHeader's rules around the seal, or CalcDifficulty alone: one launch per call */
#define GSV_K_BLOCK_MERGE 25  /* the merge of the pre-seal, seal and post-seal statuses: one launch per call */
#define GSV_K_SUMMIT 26
/* Ids added behind GSV_K_SUMMIT (pinned like the seven before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_CREST. */
#define GSV_K_RECEIPT_SCAN 26  /* receipts: the strict decode, one descriptor per bloom item: one launch per call */
#define GSV_K_RECEIPT_BLOOM 27 /* receipts: one Keccak-256 per log address and topic, the bloom rows: one launch */
#define GSV_K_RECEIPT_LISTS 28 /* receipts: each list's first failure and gas used: one launch per call */
#define GSV_K_RECEIPT_CHECK 29 /* receipts: gas used, bloom and root against the header's: one launch per call */
#define GSV_K_BLOOM9 30        /* bloom9 over byte strings: one launch per call */
#define GSV_K_CREST 31
/* Ids added behind GSV_K_CREST (pinned like the eight before it); gsv_ctx_kernel_time takes every id below
 * GSV_K_RIDGE. */
#define GSV_K_BLOOMBITS_GENERATE 31 /* bloombits: the section transposition, one launch per call */
#define GSV_K_BITSET_COMPRESS 32    /* bitutil.CompressBytes over n vectors: one launch per call */
#define GSV_K_BITSET_DECOMPRESS 33  /* bitutil.DecompressBytes over n vectors: one launch per call */
#define GSV_K_BLOOMBITS_MATCH 34    /* bloombits: the match bitsets and counts, one launch per call */
#define GSV_K_BLOOMBITS_TOTALS 35   /* bloombits blocks: each query's total, one launch per call */
#define GSV_K_BLOOMBITS_SCAN 36     /* bloombits blocks: the totals scanned into block_off, one launch per call */
#define GSV_K_BLOOMBITS_BLOCKS 37   /* bloombits blocks: the block numbers, one launch per call */
#define GSV_K_BLOOM_FILTER 38       /* bloomFilter over plain blooms: one launch per call */
#define GSV_K_RIDGE 39
/* total milliseconds and launch count accumulated for kernel `kid` since the last reset */
int gsv_ctx_kernel_time(gsv_ctx *ctx, int kid, double *total_ms, long *launches);
int gsv_ctx_reset_timing(gsv_ctx *ctx);
/* prepared *_dev shapes currently cached and their device bytes */
int gsv_ctx_prepared_shapes(gsv_ctx *ctx, size_t *count, size_t *device_bytes);
/* Pipeline depth D (1..GSV_MAX_PIPELINE_DEPTH, default 1) of the shapes prepared from now on: each
 * holds D instances of its device memory (tables and workspace), so *_dev calls of ONE shape on up to
 * D different streams run concurrently instead of being ordered after each other (a stream keeps
 * the instance it last used).  A shape prepared at a lower depth is replaced by its next prepare
 * (including the implicit prepare of a binding's *_dev wrapper): the new, deeper shape serves the
 * later calls, and the old one is retired, not freed — its memory stays valid (a HIP graph captured
 * from it can still be replayed) until the shape cache's LRU bound evicts it, after its queued work.
 * Use: validating consecutive batches of equal shape on two streams overlaps one batch's
 * latency-bound tail (trie top, final exponentiation) with the next batch's bulk kernels. */
#define GSV_MAX_PIPELINE_DEPTH 8
int gsv_ctx_set_pipeline_depth(gsv_ctx *ctx, int depth);
/* A stream for a pipelining caller, on a hardware (HSA) queue of its own.  HIP multiplexes ordinary
 * streams over GPU_MAX_HW_QUEUES (4) in-order queues, so two of a caller's streams can share one, and
 * batches issued on them then run one after the other (including every event wait placed on them): a
 * pipeline of D batches needs D streams on D queues.  The stream is created with a CU mask of every CU
 * of the context's device (hipExtStreamCreateWithCUMask: HIP backs such a stream by a dedicated queue);
 * it is ordered with the legacy NULL stream like a hipStreamDefault stream (a BLOCKING stream).
 * The context owns the stream: at most GSV_MAX_STREAMS are live per context (the next create returns
 * GSV_E_INVALID_ARG: more queues oversubscribe the hardware scheduler), gsv_stream_destroy (after the
 * stream's work) releases one and refuses a stream this context did not create, and gsv_ctx_destroy
 * destroys those still live, so a process that exits without destroying its streams tears nothing down
 * in the runtime's static-destructor order. */
#define GSV_MAX_STREAMS 8
int gsv_stream_create(gsv_ctx *ctx, void **stream_out);
int gsv_stream_destroy(gsv_ctx *ctx, void *stream);
/* Live dedicated-queue streams of the context: the caller's (gsv_stream_create) and the prepared
 * shapes' side streams.  A prepared notary shape (and the notary partition) forks its chunk roots onto
 * side streams of its OWN, one per pipeline instance, each a blocking stream on a queue of its own, freed
 * when the shape is evicted or retired.  At most 8 side streams are live per context: a prepare past
 * that takes them from the least recently used shapes holding some, which then run their chunk roots
 * after their transactions on the caller's stream until prepared again (same results; the prepare
 * succeeds; a shape whose side stream has a graph capture open keeps it). */
int gsv_ctx_stream_count(gsv_ctx *ctx, int *user_streams, int *side_streams);

/* ---- Keccak-256 (A10) ----
 * Message i is data[off[i] .. off[i+1]); out32[32*i .. +32) = Keccak256(message i). */
int gsv_keccak256_batch(gsv_ctx *ctx, const uint8_t *data, const uint64_t *off, size_t n,
                        uint8_t *out32);
int gsv_keccak256_batch_dev(gsv_ctx *ctx, const uint8_t *d_data, const uint64_t *d_off, size_t n,
                            uint8_t *d_out32, void *stream);

/* ---- SHA-256 and RIPEMD-160: the sha256hash (0x02) and ripemd160hash (0x03) precompiles ----
 * Message i is data[off[i] .. off[i+1]), as for gsv_keccak256_batch; n == 0 is a success that launches
 * nothing.  Neither hash can fail per item, so there is no status output.
 *   sha256:    out32[32*i .. +32) = SHA-256(message i) (core/vm/contracts.go:114-117).
 *   ripemd160: out32[32*i .. +32) = the precompile's row (contracts.go:129-133): 12 zero bytes, then the
 *              20-byte RIPEMD-160 digest of message i (common.LeftPadBytes(.., 32)).  The plain digest is
 *              bytes 12 .. 32 of the row; there is no 20-byte form.
 * The host forms stage, run and copy back.  The _dev forms take device arrays (the n + 1 offsets
 * included), any byte alignment of d_data and d_out32, and only enqueue one launch (GSV_K_SHA256 /
 * GSV_K_RIPEMD160) on `stream` (NULL = the context stream): no allocation, no synchronisation, no
 * prepare call, capturable.  They read no byte outside d_data[d_off[0] .. d_off[n]) but for the other
 * bytes of the aligned dwords that hold its first and its last byte. */
int gsv_sha256_batch(gsv_ctx *ctx, const uint8_t *data, const uint64_t *off, size_t n, uint8_t *out32);
int gsv_sha256_batch_dev(gsv_ctx *ctx, const uint8_t *d_data, const uint64_t *d_off, size_t n,
                         uint8_t *d_out32, void *stream);
int gsv_ripemd160_batch(gsv_ctx *ctx, const uint8_t *data, const uint64_t *off, size_t n, uint8_t *out32);
int gsv_ripemd160_batch_dev(gsv_ctx *ctx, const uint8_t *d_data, const uint64_t *d_off, size_t n,
                            uint8_t *d_out32, void *stream);

/* ---- secp256k1 public-key recovery (A5-A9) ----
 * msg32: n x 32 B message hashes; sig65: n x 65 B [R || S || recid].
 * pub65_out: n x 65 B uncompressed keys (0x04 || X || Y), zeroed for failed items.  The call also uses
 * pub65_out as working storage until it completes.
 * status: GSV_ST_OK / GSV_ST_INVALID_RECID (recid >= 4) / GSV_ST_RECOVER_FAILED.
 * addr20_out (optional, may be NULL): Keccak256(X || Y)[12:32] for OK items. */
int gsv_ecrecover_batch(gsv_ctx *ctx, const uint8_t *msg32, const uint8_t *sig65, size_t n,
                        uint8_t *pub65_out, uint8_t *addr20_out, uint8_t *status);
int gsv_ecrecover_batch_dev(gsv_ctx *ctx, const uint8_t *d_msg32, const uint8_t *d_sig65, size_t n,
                            uint8_t *d_pub65_out, uint8_t *d_addr20_out, uint8_t *d_status,
                            void *stream);

/* ---- ECDSA verification with a known key, and public-key parsing ----
 * The cgo path's semantics (crypto/secp256k1/ext.h, secp256.go:124-169), not signature_nocgo.go's.
 * msg32: n x 32 B hashes; sig64: n x 64 B [R || S]; key i = pub[pub_off[i] .. pub_off[i+1]), any length.
 * ok[i] = 1 iff all of
 *   - r, s in [1, n) (a value >= n is invalid, not reduced) and s <= n/2 (the malleability rule);
 *   - the key parses (eckey_pubkey_parse): 33 bytes 02|03 || X with X < p, X^3 + 7 a square, Y of that
 *     parity; or 65 bytes 04|06|07 || X || Y with X, Y < p, Y^2 = X^3 + 7 and, for 06|07, Y of the
 *     prefix's parity; every other length or prefix is invalid;
 *   - with m = msg mod n (m = 0 is allowed), X = (m/s) G + (r/s) P is not the identity and its x
 *     coordinate is r, or r + n when r < p - n.
 * Else ok[i] = 0: an item never fails the batch.
 * gsv_pubkey_parse_batch applies the key rule alone and re-encodes: pub65_out[i] = 04 || X || Y
 * (canonical) and ok[i] = 1, or 65 zero bytes and ok[i] = 0 (secp256k1_ext_reencode_pubkey with a
 * 65-byte output: DecompressPubkey; CompressPubkey is its first 33 bytes with 02 | (Y & 1)). */
int gsv_ecdsa_verify_batch(gsv_ctx *ctx, const uint8_t *msg32, const uint8_t *sig64, const uint8_t *pub,
                           const uint64_t *pub_off, size_t n, uint8_t *ok);
int gsv_pubkey_parse_batch(gsv_ctx *ctx, const uint8_t *pub, const uint64_t *pub_off, size_t n,
                           uint8_t *pub65_out, uint8_t *ok);
/* Device-resident forms.  Keys in the device layout: d_pub65 = n rows of 65 B (a 33-byte key in the
 * first 33 bytes of its row; the rest of that row is not read as key material), d_publen = n length
 * bytes, 33 or 65 (any other value: an invalid key, as the host forms give every other length).  They
 * only enqueue (one launch) on `stream` (NULL = the context stream).  No prepare call. */
int gsv_ecdsa_verify_batch_dev(gsv_ctx *ctx, const uint8_t *d_msg32, const uint8_t *d_sig64,
                               const uint8_t *d_pub65, const uint8_t *d_publen, size_t n, uint8_t *d_ok,
                               void *stream);
int gsv_pubkey_parse_batch_dev(gsv_ctx *ctx, const uint8_t *d_pub65, const uint8_t *d_publen, size_t n,
                               uint8_t *d_pub65_out, uint8_t *d_ok, void *stream);

/* ---- crypto.Sign and public-key derivation ----
 * secp256k1.Sign (crypto/secp256k1/secp256.go:70-99): msg32 = n x 32 B hashes, seckey32 = n x 32 B
 * big-endian secret keys.  A key of 0 or >= n gets status GSV_ST_INVALID_KEY (secp256k1_ec_seckey_verify,
 * secp256.go:78) and 65 zero bytes.  Else status GSV_ST_OK and sig65_out[i] = [R || S || recid], byte
 * for byte what the reference returns: the nonce is RFC 6979's (HMAC-SHA256 over key || msg32, the
 * message as its raw 32 bytes; secp256k1_nonce_function_rfc6979 with no extra data), tried at counter
 * 0, 1, ... until it is in [1, n) and gives r, s != 0; s is normalised to the low half; recid =
 * (R.x >= n ? 2 : 0) | (R.y odd), bit 0 flipped when s was negated.  secp256k1.ErrSignFailed has no
 * status: with this nonce function the reference cannot return it.
 * gsv_pubkey_create_batch applies the same key rule: pub65_out[i] = 04 || X || Y of key i's point and,
 * when addr20_out is not NULL, addr20_out[i] = Keccak256(X || Y)[12:32]; zero bytes for an invalid key.
 *
 * Secret keys.  The host forms stage the keys in the context's device arena and overwrite that copy,
 * on the context stream and before their final synchronisation, on every return that follows the
 * copy-in (error returns included); they keep no host copy.  The _dev forms read the caller's device
 * buffer and write no key material anywhere; wiping that buffer is the caller's.
 * What this path does NOT promise (compare crypto/signature_cgo.go:48-51 on its own caveat): the
 * fixed-base multiplication indexes a 1 GB table in HBM by 20-bit digits of the secret nonce (and, for
 * key derivation, of the secret key), and the low-s step branches on a bit derived from secrets;
 * libsecp256k1's ecmult_gen is blinded and scans its whole table.  So the path is NOT hardened against a
 * co-tenant that observes timing or memory traffic on the same GPU.  The nonce's inversion mod n is the
 * constant-time one.  Nor does the library control what the HIP runtime's own host-to-device staging
 * buffer holds after a copy from pageable memory. */
int gsv_ecdsa_sign_batch(gsv_ctx *ctx, const uint8_t *msg32, const uint8_t *seckey32, size_t n,
                         uint8_t *sig65_out, uint8_t *status);
int gsv_pubkey_create_batch(gsv_ctx *ctx, const uint8_t *seckey32, size_t n, uint8_t *pub65_out,
                            uint8_t *addr20_out, uint8_t *status);
/* Device-resident forms: every array in HBM (d_addr20_out may be NULL).  They only enqueue (one launch)
 * on `stream` (NULL = the context stream).  No prepare call. */
int gsv_ecdsa_sign_batch_dev(gsv_ctx *ctx, const uint8_t *d_msg32, const uint8_t *d_seckey32, size_t n,
                             uint8_t *d_sig65_out, uint8_t *d_status, void *stream);
int gsv_pubkey_create_batch_dev(gsv_ctx *ctx, const uint8_t *d_seckey32, size_t n, uint8_t *d_pub65_out,
                                uint8_t *d_addr20_out, uint8_t *d_status, void *stream);
/* ---- ScalarMult and ECDH shared secrets ----
 * secp256k1_ext_scalar_mul (crypto/secp256k1/ext.h:104-142) behind BitCurve.ScalarMult (curve.go:221-259):
 * point64 = n x 64 B points X || Y (big-endian), scalar32 = n x 32 B big-endian scalars k.
 *   - A scalar of 0 or >= n gets status GSV_ST_INVALID_KEY and a zero row: the reference returns 0 and
 *     leaves its buffer alone, which Go turns into (nil, nil) and ecies.GenerateShared into
 *     ErrSharedKeyIsPointAtInfinity.  This rule is tested first: it is the reference's only failure.
 *   - A coordinate >= p is accepted and reduced mod p (fe_set_b32's verdict is ignored in ext.h).
 *   - Else status GSV_ST_OK and point64_out[i] = X || Y of the affine k P, byte for byte the reference's.
 *   - THE ONE DIVERGENCE.  A point with Y^2 != X^3 + 7 (after the reduction) and a scalar in range gets
 *     status GSV_ST_INVALID_CURVE and a zero row.  The reference returns 1 and the output of its addition
 *     formulas on another curve y^2 = x^3 + b'; orders there are not n, ecmult_const assumes no
 *     exceptional case, and the ladder here is only correct for a point of order n, so that value is an
 *     artefact nobody should consume: ecies.Decrypt checks IsOnCurve before it multiplies (ecies.go:337),
 *     as p2p/discover and discv5 do on the keys they parse.  The status mirrors ecies.ErrInvalidCurve.
 * gsv_ecdh_batch is the same multiplication of public point pub64[i] by secret key seckey32[i], under the
 * same three statuses, and returns what ECIES makes of its X:
 *   shared32_out (may be NULL): X, 32 bytes, left-padded with zeros: GenerateShared(pub, 16, 16);
 *   keys48_out (may be NULL): Ke || Km of ECIES_AES128_SHA256 (crypto/ecies/params.go:69-76) with s1
 *     empty, as ecies.Encrypt(rand, pub, m, nil, nil) and RLPx derive them: K = SHA256(00 00 00 01 || X)
 *     (concatKDF, ecies.go:167-192), Ke = K[0:16], Km = SHA256(K[16:32]) (ecies.go:273-277).
 * At least one of the two is asked for (both NULL with n > 0: GSV_E_INVALID_ARG).  Every output row of
 * a failed item is zero bytes.
 *
 * Secrets: the scalar, the product point ("usually secret", ext.h:109), the shared X and the derived
 * keys.  The host forms stage all of them FIRST in the context's device arena, contiguous from offset 0,
 * and overwrite that whole region on the context stream, before their final synchronisation, on every
 * return that follows the copy-in (error returns included); the public points and the status bytes
 * behind it are left.  The _dev forms write secrets only to the caller's output buffers.
 * What this path does NOT promise, beyond the caveat of the Sign block above: the GLV ladder's table of
 * odd multiples (LDS and a private array) is indexed by 4-bit digits of the secret scalar, and the
 * ladder's exceptional-case guards are wave-uniform tests on values derived from secrets, so a rare
 * case in one lane costs its whole wave time.  libsecp256k1's ecmult_const is constant-time.  This
 * path is NOT hardened against a co-tenant that observes timing or memory traffic on the same GPU.  The
 * inversion of Z mod p is the constant-time one, and no lane leaves the schedule early. */
int gsv_secp256k1_scalar_mul_batch(gsv_ctx *ctx, const uint8_t *point64, const uint8_t *scalar32, size_t n,
                                   uint8_t *point64_out, uint8_t *status);
int gsv_ecdh_batch(gsv_ctx *ctx, const uint8_t *pub64, const uint8_t *seckey32, size_t n,
                   uint8_t *shared32_out, uint8_t *keys48_out, uint8_t *status);
/* Device-resident forms: every array in HBM (one of d_shared32_out, d_keys48_out may be NULL).  They only
 * enqueue (one launch) on `stream` (NULL = the context stream).  No prepare call. */
int gsv_secp256k1_scalar_mul_batch_dev(gsv_ctx *ctx, const uint8_t *d_point64, const uint8_t *d_scalar32,
                                       size_t n, uint8_t *d_point64_out, uint8_t *d_status, void *stream);
int gsv_ecdh_batch_dev(gsv_ctx *ctx, const uint8_t *d_pub64, const uint8_t *d_seckey32, size_t n,
                       uint8_t *d_shared32_out, uint8_t *d_keys48_out, uint8_t *d_status, void *stream);
/* Test hook of the rule on secret keys: copies bytes [off, off + n) of the context's staging arena, as
 * they are now, to `out` (GSV_E_INVALID_ARG past the arena's end).  The host forms above stage their
 * secrets from offset 0. */
int gsv_ctx_arena_read(gsv_ctx *ctx, size_t off, size_t n, uint8_t *out);

/* ---- ecies.Encrypt and PrivateKey.Decrypt (crypto/ecies/ecies.go:246-366) ----
 * The whole of both for ECIES_AES128_SHA256 (params.go:69-76), byte for byte the reference's: the key
 * agreement of gsv_ecdh_batch, then AES-128-CTR and the HMAC-SHA256 tag.  s1 (the KDF's shared
 * information) is always empty and is not a parameter: every caller in the reference passes nil.  s2
 * (the MAC's, e.g. RLPx's EIP-8 size prefix) is per item: item i's is s2[s2_off[i] .. s2_off[i+1]);
 * s2 and s2_off both NULL means every s2 is empty.  An item of 2^32 bytes or more: GSV_E_TOO_LARGE.
 *
 * Decrypt.  Item i is c = ct[ct_off[i] .. ct_off[i+1]).  The checks run in the reference's order and the
 * first failure decides the status:
 *    1. len(c) == 0                                  GSV_ST_INVALID_MESSAGE
 *    2. c[0] not 2, 3 or 4                           GSV_ST_INVALID_PUBKEY, whatever the length
 *    3. len(c) < 98                                  GSV_ST_INVALID_MESSAGE
 *    4. c[0] is 2 or 3                               GSV_ST_INVALID_PUBKEY: rLen is 65 for all three, and
 *                                                    elliptic.Unmarshal takes only 04 || X || Y
 *    5. X or Y >= p                                  GSV_ST_INVALID_PUBKEY.  A decision, not a reading: what
 *       elliptic.Unmarshal does with such a coordinate depends on the Go release, and that code is not in
 *       the reference tree.  No release yields a different plaintext; refusing is the strict reading.
 *    6. Y^2 != X^3 + 7                               GSV_ST_INVALID_CURVE (ecies.go:337)
 *    7. secret key 0 or >= n                         GSV_ST_INVALID_KEY
 *    8. 98 <= len(c) < 113                           GSV_ST_INVALID_MESSAGE.  em is shorter than an IV: the
 *       reference fails the tag there or, with a matching tag, panics in symDecrypt.
 *    9. tag != HMAC-SHA256(Km, c[65 : len-32] || s2) GSV_ST_INVALID_MESSAGE
 *   10. else GSV_ST_OK: the message is c[81 : len-32] XOR the AES-128-CTR keystream of Ke from the counter
 *       block c[65:81], which is Go's cipher.NewCTR: one 128-bit big-endian integer, incremented with
 *       carry through all 16 bytes.  len(c) == 113 is a valid empty message.
 * Item i owns the slot msg_out[ct_off[i] .. ct_off[i+1]), and the call writes every byte of it: the
 * message, then zeros; msg_len[i] = len(c) - 113.  A failed item's slot is all zeros and its msg_len 0;
 * no plaintext byte of an item whose tag failed is left anywhere the call wrote.  msg_out does not
 * overlap ct.
 *
 * Encrypt, with the two things the reference draws from rand supplied by the caller: the ephemeral
 * secret key and the IV.  Item i: m = msg[msg_off[i] .. msg_off[i+1]) to the point pub64[i] (X || Y):
 *   ct_i = 04 || eph G || iv || CTR(Ke, iv, m) || HMAC-SHA256(Km, iv || CTR(..) || s2),
 * written at ct_out + msg_off[i] + 113 i (GSV_ECIES_OVERHEAD = 65 + 16 + 32, eciesOverhead of
 * p2p/rlpx.go:58).  An ephemeral key of 0 or >= n gets GSV_ST_INVALID_KEY; else a recipient point off
 * the curve GSV_ST_INVALID_CURVE (gsv_ecdh_batch's divergence: the reference's Encrypt does not check);
 * else an empty message GSV_ST_INVALID_MESSAGE (the reference returns (nil, nil), ecies.go:280).  A
 * failed item's 113 + len(m) bytes are zeros.
 *
 * Secrets: the secret and ephemeral keys, Ke || Km and the plaintext.  The host forms stage them FIRST
 * in the context's device arena (keys, the work area, the plaintext), contiguous from offset 0, and
 * overwrite that region on the context stream, before their final synchronisation, on every return
 * that follows the copy-in (error returns included).  The caveats of the Sign and ECDH blocks above
 * hold, and one more: the AES tables are indexed by key-dependent bytes. */
#define GSV_ECIES_OVERHEAD 113
int gsv_ecies_decrypt_batch(gsv_ctx *ctx, const uint8_t *ct, const uint64_t *ct_off, const uint8_t *seckey32,
                            const uint8_t *s2, const uint64_t *s2_off, size_t n, uint8_t *msg_out,
                            uint32_t *msg_len, uint8_t *status);
int gsv_ecies_encrypt_batch(gsv_ctx *ctx, const uint8_t *msg, const uint64_t *msg_off, const uint8_t *pub64,
                            const uint8_t *eph_seckey32, const uint8_t *iv16, const uint8_t *s2,
                            const uint64_t *s2_off, size_t n, uint8_t *ct_out, uint8_t *status);
/* Device-resident forms: every array in HBM, the offset tables included (as for gsv_keccak256_batch_dev);
 * every item shorter than 2^32 bytes (not checked).  They only enqueue on `stream` (NULL = the context
 * stream) and allocate nothing; no prepare call; capturable into a HIP graph.  Decrypt is three
 * launches: the checks that precede the ladder (they also gather R out of the ciphertexts, which the
 * ladder reads as rows), the ladder of gsv_ecdh_batch_dev, and the symmetric kernel (timed as
 * GSV_K_ECIES; the first two as GSV_K_ECRECOVER).  Encrypt is three as well: gsv_pubkey_create_batch_dev's
 * launch for eph G, the ladder, the symmetric kernel.
 * d_work: gsv_ecies_work_bytes(n, encrypt) bytes of the caller's.  The launches hand each other the
 * derived keys (and R) there; the symmetric kernel overwrites all of it with zeros before it ends.
 * d_status is written twice in Decrypt (the early checks, then the final status). */
size_t gsv_ecies_work_bytes(size_t n, int encrypt);
int gsv_ecies_decrypt_batch_dev(gsv_ctx *ctx, const uint8_t *d_ct, const uint64_t *d_ct_off,
                                const uint8_t *d_seckey32, const uint8_t *d_s2, const uint64_t *d_s2_off, size_t n,
                                uint8_t *d_msg_out, uint32_t *d_msg_len, uint8_t *d_status, uint8_t *d_work,
                                void *stream);
int gsv_ecies_encrypt_batch_dev(gsv_ctx *ctx, const uint8_t *d_msg, const uint64_t *d_msg_off,
                                const uint8_t *d_pub64, const uint8_t *d_eph_seckey32, const uint8_t *d_iv16,
                                const uint8_t *d_s2, const uint64_t *d_s2_off, size_t n, uint8_t *d_ct_out,
                                uint8_t *d_status, uint8_t *d_work, void *stream);

/* ---- the ecrecover precompile (core/vm/contracts.go:78-101) ----
 * Input i = in[off[i] .. off[i+1]) = hash(32) || v(32) || r(32) || s(32), right-padded with zeros to
 * 128 bytes (longer inputs: only the first 128 bytes are read).  ok[i] = 1 and out32[i] =
 * LeftPadBytes(Keccak256(pub[1:])[12:], 32) on success; ok[i] = 0 and out32[i] zero where the
 * reference returns (nil, nil): input[32:63] not all zero, ValidateSignatureValues(v - 27, r, s,
 * homestead = false) false (crypto/crypto.go:181-192), or recovery failing. */
int gsv_ecrecover_precompile_batch(gsv_ctx *ctx, const uint8_t *in, const uint64_t *off, size_t n,
                                   uint8_t *out32, uint8_t *ok);
/* Device-resident form over padded records: d_in128 = n x 128 bytes in HBM. */
int gsv_ecrecover_precompile_batch_dev(gsv_ctx *ctx, const uint8_t *d_in128, size_t n, uint8_t *d_out32,
                                       uint8_t *d_ok, void *stream);

/* ---- recoverPlain (A4): sighash + (R, S, V) -> sender address ----
 * r32/s32: n x 32 B big-endian; v: per-item V already reduced by the signer
 * (27/28 for Homestead/Frontier, tx.V - 2*chainId - 8 for EIP-155) as a uint64 with
 * v_big[i] != 0 meaning "V had more than 8 bits" (-> GSV_ST_INVALID_SIG).
 * homestead: 1 = reject s > n/2 (crypto/crypto.go:188). */
int gsv_sender_batch(gsv_ctx *ctx, const uint8_t *sighash32, const uint8_t *r32, const uint8_t *s32,
                     const uint64_t *v, const uint8_t *v_big, size_t n, int homestead,
                     uint8_t *addr20_out, uint8_t *status);

/* ---- types.Sender over RLP-encoded transactions (A1-A4) ----
 * tx i = rlp[off[i] .. off[i+1]); chain_id big-endian (len 0 = 0). */
int gsv_tx_sender_batch(gsv_ctx *ctx, const uint8_t *rlp, const uint64_t *off, size_t n,
                        const uint8_t *chain_id, size_t chain_id_len, int signer_kind,
                        uint8_t *addr20_out, uint8_t *status);

/* ---- types.SignTx over RLP-encoded transactions ----
 * types.SignTx(tx, signer, prv) (core/types/transaction_signing.go:56-63): h = signer.Hash(tx), sig =
 * crypto.Sign(h, prv), tx.WithSignature(signer, sig), for a batch.  The inverse of gsv_tx_sender_batch.
 * Input.  tx i = rlp[off[i] .. off[i+1]) = rlp.EncodeToBytes(tx), signed or not: the nine-item list
 *   [nonce, price, gas, to, value, data, V, R, S] (core/types/transaction.go:55-70); an unsigned
 *   NewTransaction carries V = R = S = 0 as three 0x80 bytes.  seckey32 = n x 32 B big-endian secret keys.
 *   One signer kind and one chain id (big-endian, length 0 = 0, at most 64 bytes, leading zero bytes
 *   ignored) for the whole call.
 * Decode.  The rules of gsv_tx_sender_batch (rlp/decode.go for txdata); what rlp.DecodeBytes refuses gets
 *   GSV_ST_BAD_RLP.  The incoming V, R and S only have to decode (decodeBigInt, rlp/decode.go:271-287: any
 *   length, no leading zero byte); their values are ignored: SignTx on a signed transaction signs it again
 *   (transaction_signing_test.go:124), so what gsv_tx_sender_batch rejects as INVALID_SIG,
 *   INVALID_CHAIN_ID or RECOVER_FAILED signs normally here.
 * Hash.  EIP155Signer.Hash (:155-165): Keccak-256 of rlp([six fields, chainId, 0, 0]); FrontierSigner.Hash
 *   (:207-216, HomesteadSigner's too): of rlp([six fields]).  A nil recipient that came as 0xc0 is hashed, and
 *   written out, as 0x80 (rlp.Encode of the decoded struct, rlp/encode.go:552-559).
 * Signature.  gsv_ecdsa_sign_batch's, byte for byte (RFC 6979 nonce, low s, recovery id); a key of 0 or
 *   >= n gets GSV_ST_INVALID_KEY.
 * Signature values (:141-151, :195-203).  R and S the 32-byte halves as big integers (leading zero bytes
 *   dropped).  Frontier, Homestead, and EIP-155 with chain id 0: V = recid + 27 (the EIP-155 hash still
 *   carries chainId = 0 as 0x80).  EIP-155 with another chain id: V = recid + 35 + 2 chainId, up to 65 bytes.
 * Output.  rlp.Encode of the signed transaction in slot i, which starts at out + off[i] + i * G with
 *   G = GSV_TX_SIGN_GROWTH(chain_id_len) and is as long as the input plus G, so `out` holds off[n] + n * G
 *   bytes and neither a scan nor a layout call is needed.  out_len[i] = the encoding's length; txhash32_out
 *   (may be NULL) = tx.Hash() = Keccak-256 of those bytes (transaction.go:198-206).
 * Status precedence: GSV_ST_BAD_RLP before GSV_ST_INVALID_KEY (the reference decodes before it signs).
 * The one deviation: an item longer than 2^20 bytes gets GSV_ST_BODY_TOO_LARGE, whatever it holds, and is
 *   not signed; it could never enter a collation (sharding/collation.go:45, 169-171).
 * A failed item has out_len 0 and a zero hash, and no byte of its slot is written.  No byte outside
 *   [slot, slot + out_len[i]) is written for any item.
 *
 * GSV_TX_SIGN_GROWTH(chain_id_len): the signed encoding of item i is never longer than len_i + G.  The
 * decode rules leave the six fields one encoding, so they keep their length (0xc0 -> 0x80 is one byte for
 * one); the input's V, R, S are at least 1 byte each; the output's V is at most chain_id_len + 1 bytes
 * of integer behind at most 2 of header, R and S at most 1 + 32 each: the payload grows by at most
 * (chain_id_len + 3 - 1) + 2 * (33 - 1) = chain_id_len + 66 <= 130 bytes.  The input's list header is the
 * canonical one for its payload (the decoder refuses another); a payload below 56 bytes grows to below
 * 256 and one below 2^16 to below 2^24, so the header grows by at most 1 byte: G = chain_id_len + 67.
 *
 * Secret keys: as gsv_ecdsa_sign_batch states above.  The host form stages the keys FIRST in the
 * context's device arena and overwrites that copy on the context stream before its final
 * synchronisation, on every return that follows the copy-in; the _dev form reads the caller's buffer and
 * writes no key material anywhere (d_work holds hashes, signatures and offsets).  The same caveat on
 * side channels holds: this path is NOT hardened against a co-tenant observing timing or memory traffic.
 *
 * Argument errors, before any HIP call: GSV_E_INVALID_ARG for a NULL context, chain_id_len > 64, a NULL
 * chain id with a length, a signer kind that is none of GSV_SIGNER_*. */
#define GSV_TX_SIGN_GROWTH(chain_id_len) ((size_t)(chain_id_len) + 67)
int gsv_tx_sign_batch(gsv_ctx *ctx, const uint8_t *rlp, const uint64_t *off, size_t n, const uint8_t *seckey32,
                      const uint8_t *chain_id, size_t chain_id_len, int signer_kind, uint8_t *out,
                      uint32_t *out_len, uint8_t *txhash32_out, uint8_t *status);
/* Device-resident form: every array in HBM, d_off = n + 1 ascending uint64 offsets into d_rlp as in
 * gsv_keccak256_batch_dev (slot i at d_out + d_off[i] + i * G), d_out_len n x uint32, d_txhash32_out may
 * be NULL (else 4-byte aligned), d_work = gsv_tx_sign_work_bytes(n) bytes of the caller's, 16-byte
 * aligned.  It only enqueues on `stream` (NULL = the context stream): three launches, k_tx_sighash
 * (GSV_K_TX_SIGHASH), the signature kernel of gsv_ecdsa_sign_batch_dev (GSV_K_ECRECOVER), k_tx_seal
 * (GSV_K_TX_SEAL), handing each other hashes, signatures and a 16-byte record per item through d_work.
 * No allocation, no synchronisation, no prepare call: the chain id travels as kernel arguments. */
size_t gsv_tx_sign_work_bytes(size_t n);
int gsv_tx_sign_batch_dev(gsv_ctx *ctx, const uint8_t *d_rlp, const uint64_t *d_off, size_t n,
                          const uint8_t *d_seckey32, const uint8_t *chain_id, size_t chain_id_len,
                          int signer_kind, uint8_t *d_out, uint32_t *d_out_len, uint8_t *d_txhash32_out,
                          uint8_t *d_status, uint8_t *d_work, void *stream);

/* ---- collation chunk root (B1-B5) ----
 * body i = bodies[off[i] .. off[i+1]), each <= 2^20 bytes (else GSV_E_TOO_LARGE).
 * root32_out[i] = DeriveSha(Chunks(body i)); an empty body gives emptyRoot. */
int gsv_chunk_root_batch(gsv_ctx *ctx, const uint8_t *bodies, const uint64_t *off, size_t n,
                         uint8_t *root32_out);
/* Prepares gsv_chunk_root_batch_dev for exactly these host offsets h_off[0..n] (trie plans per body
 * length, device offset table, workspace). */
int gsv_chunk_root_prepare(gsv_ctx *ctx, const uint64_t *h_off, size_t n);
int gsv_chunk_root_batch_dev(gsv_ctx *ctx, const uint8_t *d_bodies, const uint64_t *h_off, size_t n,
                             uint8_t *d_root32_out, void *stream);

/* ---- BN254 pairing check (C1-C6) ----
 * check i = in[off[i] .. off[i+1]) in the precompile encoding (k x 192 B);
 * verdict[i] = GSV_PAIRING_TRUE / FALSE / BAD_INPUT. */
int gsv_bn256_pairing_check_batch(gsv_ctx *ctx, const uint8_t *in, const uint64_t *off, size_t n,
                                  uint8_t *verdict);
/* Device-resident form: d_in in HBM, h_off on the host (n+1 offsets into d_in), d_verdict in HBM.
 * Enqueues on `stream` (NULL = the context stream); returns after the launches are queued.
 * gsv_bn256_pairing_prepare builds the lane tables for exactly these offsets. */
int gsv_bn256_pairing_prepare(gsv_ctx *ctx, const uint64_t *h_off, size_t n);
int gsv_bn256_pairing_check_batch_dev(gsv_ctx *ctx, const uint8_t *d_in, const uint64_t *h_off, size_t n,
                                      uint8_t *d_verdict, void *stream);

/* ---- BN254 G1 addition and scalar multiplication: the bn256Add (0x06) and bn256ScalarMul (0x07)
 * precompiles (core/vm/contracts.go:274-312) ----
 * Input i = in[off[i] .. off[i+1]), right-padded with zeros to the record size and cut there (getData,
 * core/vm/common.go:37-47): add = x1 || y1 || x2 || y2 (128 B), scalar mul = x || y || k (96 B), 32-byte
 * big-endian words.  A point decodes as G1.Unmarshal does (bn256.go:120-158): every coordinate < p (a
 * coordinate equal to p is an error), (0, 0) is the point at infinity, anything else must satisfy
 * y^2 = x^3 + 3.  status[i] = GSV_ST_BN_BAD_INPUT and 64 zero bytes where the reference returns the
 * unmarshal error (whatever k is); else GSV_ST_OK and out64[i] = Marshal(P1 + P2) / Marshal(k P) for any
 * k in [0, 2^256): the affine point, 64 zero bytes for infinity.  So an empty input is OK with 64 zero
 * bytes.  No prepare call. */
int gsv_bn256_add_batch(gsv_ctx *ctx, const uint8_t *in, const uint64_t *off, size_t n, uint8_t *out64,
                        uint8_t *status);
int gsv_bn256_scalar_mul_batch(gsv_ctx *ctx, const uint8_t *in, const uint64_t *off, size_t n, uint8_t *out64,
                               uint8_t *status);
/* Device-resident forms over padded records: d_in128 = n x 128 B, d_in96 = n x 96 B in HBM; d_out64 =
 * n x 64 B, d_status = n bytes.  They only enqueue (one launch) on `stream` (NULL = the context stream). */
int gsv_bn256_add_batch_dev(gsv_ctx *ctx, const uint8_t *d_in128, size_t n, uint8_t *d_out64, uint8_t *d_status,
                            void *stream);
int gsv_bn256_scalar_mul_batch_dev(gsv_ctx *ctx, const uint8_t *d_in96, size_t n, uint8_t *d_out64,
                                   uint8_t *d_status, void *stream);

/* ---- modular exponentiation: the bigModExp (0x05) precompile (core/vm/contracts.go:226-252, EIP-198) ----
 * Input i = in[off[i] .. off[i+1]) exactly as the precompile receives it, every read right-padded with
 * zeros (getData, core/vm/common.go:37-47):
 *   - baseLen, expLen, modLen are the LOW 64 BITS of the 32-byte big-endian words at 0, 32 and 64
 *     (new(big.Int).SetBytes(...).Uint64(), :228-230): bytes 0..23 of a length word are ignored, and an
 *     input shorter than 96 bytes has its missing header bytes read as zeros (the empty input: 0, 0, 0).
 *   - body = input[96:] (:232-236); base, exp, mod are the big-endian values of getData(body, 0, baseLen),
 *     getData(body, baseLen, expLen), getData(body, baseLen + expLen, modLen) (:243-245).  A body shorter
 *     than declared is right-padded, which CHANGES THE VALUES (a cut modulus gets zero low bytes).
 *   - baseLen == 0 && modLen == 0: the empty output (:238-240).  mod == 0: modLen zero bytes (:247-250).
 *     Else LeftPadBytes(base.Exp(base, exp, mod).Bytes(), modLen) (:251): always exactly modLen bytes.
 *     x^0 mod m = 1 mod m (0 for m == 1), 0^0 included; the base may be longer and larger than the
 *     modulus; any modulus > 0 is legal, odd, even or a power of two.
 * The one departure: the reference would try to allocate whatever length it is told.  Here each of the
 * three lengths is capped at GSV_MODEXP_MAX_LEN bytes (the largest modulus of the reference's own vectors,
 * core/vm/contracts_test.go:36-116, and the top case of its gas formula).  An item with ANY length above the
 * cap gets status GSV_ST_MODEXP_TOO_LONG and an empty output; the batch still succeeds and the caller runs
 * that item elsewhere.  Every other item has status GSV_ST_OK.  The exponent is public: the time taken
 * depends on it.  No prepare call. */
#define GSV_MODEXP_MAX_LEN 1024
/* Host only, no context: out_off[0..n] (out_off[0] = 0; item i's output is modLen_i bytes, 0 if over the
 * cap), status[i] = GSV_ST_OK or GSV_ST_MODEXP_TOO_LONG. */
int gsv_modexp_output_layout(const uint8_t *in, const uint64_t *off, size_t n, uint64_t *out_off, uint8_t *status);
/* out is packed by out_off, which must be what gsv_modexp_output_layout gives for the same input (else
 * GSV_E_INVALID_ARG); status as there.  Items are grouped by the width class of modLen (32, 64, 128, 256,
 * 512, 1024 bytes) and each non-empty class is one call of the device form over rows left-padded with
 * zero bytes to the class's longest base, exponent and modulus.  Items with modLen == 0 and items over
 * the cap touch no device memory. */
int gsv_modexp_batch(gsv_ctx *ctx, const uint8_t *in, const uint64_t *off, size_t n, uint8_t *out,
                     const uint64_t *out_off, uint8_t *status);
/* Device-resident, one shape per call: d_in = n rows of base_len + exp_len + mod_len bytes (base || exp ||
 * mod, no 96-byte header, any byte alignment), d_out = n rows of mod_len bytes, d_work =
 * gsv_modexp_work_bytes(...) bytes of the caller's, 4-byte aligned (may be NULL when that is 0).  Only
 * enqueues, one launch (GSV_K_MODEXP), no allocation, capturable, no prepare call.  n == 0 or mod_len == 0:
 * success, nothing enqueued.  A length above the cap, or a NULL buffer where there is work:
 * GSV_E_INVALID_ARG.  No status output: every row is a legal item (mod == 0 gives zeros). */
size_t gsv_modexp_work_bytes(size_t n, uint32_t base_len, uint32_t exp_len, uint32_t mod_len);
int gsv_modexp_batch_dev(gsv_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t base_len, uint32_t exp_len,
                         uint32_t mod_len, uint8_t *d_out, uint8_t *d_work, void *stream);

/* ---- ethash (consensus/ethash): hashimotoLight, VerifySeal, dataset items, hashimotoFull, Seal ----
 * What Ethash.VerifyHeaders (consensus.go:90) spends its time in: VerifySeal (consensus.go:463-501) runs
 * hashimotoLight (algorithm.go:375) per header over the epoch's verification cache.  An epoch is 30,000
 * blocks.  The sealing half follows below the light forms, and behind it the block-header forms: the header's
 * RLP, Header.Hash() / HashNoNonce(), CalcDifficulty and the whole of Ethash.VerifyHeaders.  Not here: DAG and
 * cache files on disk, remote mining / GetWork, and pre-generating the next epoch.
 *
 * Host only, no context: cacheSize / datasetSize (algorithm.go:53-91) by the reference's formula for every
 * epoch (its 2,048-entry tables hold the same values), seedHash (algorithm.go:110-120) and generateCache
 * (algorithm.go:128-197) over cache_bytes, a multiple of 64 of at least 64 (else GSV_E_INVALID_ARG): the
 * bytes of the reference's cache on a little-endian machine, which is what the device forms read.  The
 * epoch-0 cache is 1.05 million strictly dependent permutations, under a second on one core. */
uint64_t gsv_ethash_cache_size(uint64_t block);
uint64_t gsv_ethash_dataset_size(uint64_t block);
int gsv_ethash_seed_hash(uint64_t block, uint8_t *out32);
int gsv_ethash_make_cache(const uint8_t *seed32, uint64_t cache_bytes, uint8_t *out);
/* Device-resident.  Each only enqueues one launch (GSV_K_ETHASH_ITEMS / GSV_K_ETHASH_LIGHT) on `stream`
 * (NULL = the context stream): no allocation, no synchronisation, no prepare call, capturable.  d_cache is
 * the caller's device copy of a gsv_ethash_make_cache result, 16-byte aligned; one (cache, dataset size)
 * pair per call.  GSV_E_INVALID_ARG: cache_bytes below 64 or no multiple of 64 (or 2^38 and more);
 * dataset_bytes below 128, no multiple of 128, or above 2^38 (2 parent + 1 fits 32 bits); a misaligned
 * buffer; n above 2^31 - 1.  n == 0 (count == 0): success, nothing enqueued.
 *   items:  d_out64[64 k .. +64) = generateDatasetItem(cache, first + k) (algorithm.go:232-261) for k < count,
 *           the body of generateDataset; first + count <= 2^32; d_out64 16-byte aligned.
 *   light:  (d_mix32[32 i .. +32), d_result32[32 i .. +32)) = hashimotoLight(dataset_bytes, cache,
 *           d_hash32[32 i .. +32), d_nonce[i]).  The nonce is the NUMBER (Header.Nonce.Uint64()): the kernel
 *           lays it little-endian into the seed; types.BlockNonce is its big-endian bytes.  d_hash32 4-byte
 *           and d_nonce 8-byte aligned; the outputs may have any byte alignment.
 *   verify: d_status[i] by VerifySeal's checks in its order (consensus.go:477-499), d_difficulty32 32 bytes
 *           big-endian, d_mix32 the header's MixDigest, both of any alignment:
 *             1. difficulty == 0                                    GSV_ST_INVALID_DIFFICULTY
 *             2. digest != mix                                      GSV_ST_INVALID_MIX_DIGEST
 *             3. result > floor((2^256 - 1) / difficulty)           GSV_ST_INVALID_POW
 *             4. else                                               GSV_ST_OK
 *           (3 is decided by the high half of the 512-bit product result x difficulty: no division.) */
int gsv_ethash_dataset_items_dev(gsv_ctx *ctx, const uint8_t *d_cache, uint64_t cache_bytes, uint64_t first,
                                 uint64_t count, uint8_t *d_out64, void *stream);
int gsv_ethash_light_batch_dev(gsv_ctx *ctx, const uint8_t *d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                               const uint8_t *d_hash32, const uint64_t *d_nonce, size_t n, uint8_t *d_mix32,
                               uint8_t *d_result32, void *stream);
int gsv_ethash_verify_seal_batch_dev(gsv_ctx *ctx, const uint8_t *d_cache, uint64_t cache_bytes,
                                     uint64_t dataset_bytes, const uint8_t *d_hash32, const uint64_t *d_nonce,
                                     const uint8_t *d_mix32, const uint8_t *d_difficulty32, size_t n,
                                     uint8_t *d_status, void *stream);
/* Host forms by block number: number[i] picks item i's epoch (number / 30000).  Items are grouped by epoch
 * and the results come back in input order.  Per epoch the cache is generated on the host, outside the
 * context's lock, and uploaded; a context keeps the caches of at most GSV_ETHASH_MAX_CACHES epochs, least
 * recently used out first, and frees one only inside a host call that has synchronised (never under
 * running work).  test_mode != 0 is the reference's ModeTest: a 1,024-byte cache, still seeded by the
 * epoch, and a 32 KiB dataset (ethash.go:219-221, consensus.go:485-487).  gsv_ctx_ethash_caches: how many
 * caches the context holds now. */
#define GSV_ETHASH_MAX_CACHES 3
int gsv_ethash_light_batch(gsv_ctx *ctx, const uint64_t *number, int test_mode, const uint8_t *hash32,
                           const uint64_t *nonce, size_t n, uint8_t *mix32_out, uint8_t *result32_out);
int gsv_ethash_verify_seal_batch(gsv_ctx *ctx, const uint64_t *number, const uint8_t *hash32, const uint64_t *nonce,
                                 const uint8_t *mix32, const uint8_t *difficulty32, size_t n, int test_mode,
                                 uint8_t *status);
int gsv_ctx_ethash_caches(gsv_ctx *ctx, size_t *count);
/* The sealing half: hashimotoFull (algorithm.go:393-405) and the nonce search of mine (sealer.go:97-152) over
 * the dataset itself, resident on the device: 2 permutations and 64 reads of one 128-byte page per nonce.
 * A dataset in device form is gsv_ethash_dataset_items_dev over items [0, dataset_bytes / 64) (a 2^38-byte one
 * takes two calls: first + count <= 2^32 and count < 2^32).
 *
 * Device-resident.  Each only enqueues on `stream` (NULL = the context stream): no allocation, no
 * synchronisation, no prepare call, capturable; n == 0: success, nothing enqueued.  GSV_E_INVALID_ARG:
 * dataset_bytes below 128, no multiple of 128 or above 2^38; d_dataset off 128-byte alignment (a page is one
 * cache line); hash rows off 4-byte, nonces / starts / d_nonce_out off 8-byte, d_offset off 4-byte alignment;
 * n above 2^31 - 1; span == 0 or above 2^32 - 1; n * ceil(span / 256) above 2^31 - 1 (the grid).  Rows of mix
 * digests, results and difficulties may have any byte alignment.
 *   full:    one launch (GSV_K_ETHASH_FULL): (d_mix32 row i, d_result32 row i) = hashimotoFull(dataset,
 *            d_hash32 row i, d_nonce[i]), the nonce as a NUMBER as in the light form.
 *   verify:  one launch (GSV_K_ETHASH_FULL): d_status[i] by the light form's three checks in its order.
 *   search:  a fill of d_offset with 0xFFFFFFFF (a memset node), one search launch (GSV_K_ETHASH_SEARCH) and
 *            one finish launch (GSV_K_ETHASH_FINISH).  Header h tries nonces d_start[h] + k mod 2^64 for
 *            k < span, as the reference's nonce++ wraps.  A winner has result <= floor((2^256 - 1) /
 *            difficulty), decided exactly by the 512-bit product as in verify; d_offset[h] is the SMALLEST
 *            winning k whatever the order the hardware ran them in, or 0xFFFFFFFF.  Then d_found[h] = 1,
 *            d_nonce_out[h] the winning nonce and (d_mix32, d_result32) row h its hashimotoFull; with no
 *            winner d_found[h] = 0 and the three are zeros.  A header whose difficulty is zero never wins
 *            (the reference would panic on the division).  Size span so that a launch is milliseconds:
 *            the kernels cannot be interrupted. */
int gsv_ethash_full_batch_dev(gsv_ctx *ctx, const uint8_t *d_dataset, uint64_t dataset_bytes,
                              const uint8_t *d_hash32, const uint64_t *d_nonce, size_t n, uint8_t *d_mix32,
                              uint8_t *d_result32, void *stream);
int gsv_ethash_verify_seal_full_batch_dev(gsv_ctx *ctx, const uint8_t *d_dataset, uint64_t dataset_bytes,
                                          const uint8_t *d_hash32, const uint64_t *d_nonce, const uint8_t *d_mix32,
                                          const uint8_t *d_difficulty32, size_t n, uint8_t *d_status, void *stream);
int gsv_ethash_search_dev(gsv_ctx *ctx, const uint8_t *d_dataset, uint64_t dataset_bytes, const uint8_t *d_hash32,
                          const uint8_t *d_difficulty32, const uint64_t *d_start, size_t n, uint64_t span,
                          uint32_t *d_offset, uint64_t *d_nonce_out, uint8_t *d_mix32, uint8_t *d_result32,
                          uint8_t *d_found, void *stream);
/* Host forms by block number, grouped by epoch like the light forms.  The epoch's dataset is generated on the
 * device from the epoch's cached verification cache (1 GiB at epoch 0, growing 8 MiB an epoch; test_mode: 32
 * KiB, ethash.go:294-299) and kept: a context holds at most GSV_ETHASH_MAX_DATASETS, least recently used out
 * first, freed under the caches' rule (only inside a host call that holds the lock and has synchronised).  A
 * failed allocation returns GSV_E_NOMEM and leaves the list as it was.  gsv_ctx_ethash_datasets: how many the
 * context holds now.
 *   full:  (mix32_out row i, result32_out row i) = hashimotoFull for number[i]'s epoch.
 *   seal:  per header the search above from start_nonce[i], in rounds of a bounded span (a launch stays in
 *          the milliseconds, so max_attempts is honoured to the round); a header leaves the later rounds once
 *          found, and the call ends when every header is found or has been tried max_attempts times.
 *          status[i] = GSV_ST_OK with nonce_out[i] and mix32_out row i; GSV_ST_INVALID_DIFFICULTY for a zero
 *          difficulty; GSV_ST_NONCE_NOT_FOUND (zeros) otherwise.  nonce_out[i] is the FIRST winner at or after
 *          start_nonce[i]: (nonce, mix digest) are what mine(block, id, seed = start_nonce[i], ...) reports
 *          when it runs as the only thread, whenever that nonce lies within max_attempts of the seed.
 *          Ethash.Seal with several threads returns whichever thread wins a race, each a valid seal; this is
 *          the deterministic one. */
#define GSV_ETHASH_MAX_DATASETS 2
int gsv_ethash_full_batch(gsv_ctx *ctx, const uint64_t *number, int test_mode, const uint8_t *hash32,
                          const uint64_t *nonce, size_t n, uint8_t *mix32_out, uint8_t *result32_out);
int gsv_ethash_seal_batch(gsv_ctx *ctx, const uint64_t *number, int test_mode, const uint8_t *hash32,
                          const uint8_t *difficulty32, const uint64_t *start_nonce, size_t n, uint64_t max_attempts,
                          uint64_t *nonce_out, uint8_t *mix32_out, uint8_t *status);
int gsv_ctx_ethash_datasets(gsv_ctx *ctx, size_t *count);

/* ---- block headers: Ethash.VerifyHeaders (consensus/ethash/consensus.go:90-166) over RLP-encoded headers ----
 * A chain segment goes in, header i = rlp[off[i] .. off[i+1]) as rlp.EncodeToBytes(header), and one status per
 * header comes out: verifyHeaderWorker (:152-166) and verifyHeader (:223-285) with uncle = false, the reference's
 * errors in the reference's order.  eth/downloader feeds it 2,048 headers at a time.
 *
 * Decode, as rlp.DecodeBytes into types.Header (core/types/block.go:70-86): a list of exactly 15 items;
 * ParentHash, UncleHash, Root, TxHash, ReceiptHash and MixDigest of exactly 32 bytes, Coinbase 20, Bloom 256,
 * Nonce 8; Difficulty, Number and Time big integers and GasLimit, GasUsed uint64 (no leading zero byte, at most 8
 * bytes for the two uint64); Extra a string of any length; every length in its shortest form and a single byte
 * below 0x80 as itself; no element missing or left over, no byte behind the list, no length past the input.
 * What the reference's decoder refuses is GSV_ST_BAD_RLP.  OURS, not the reference's: Difficulty and Time are
 * held in 32 bytes and Number in 8, and a header that decodes with a wider one gets GSV_ST_HEADER_TOO_WIDE.
 * An item of 2^32 bytes or more: GSV_E_TOO_LARGE from the host forms; the device forms give it GSV_ST_BAD_RLP
 * unread.
 *
 * Hashes.  Hash() is Keccak-256 of the header's RLP (block.go:101-103).  HashNoNonce() (block.go:106-122) is
 * Keccak-256 of the first 13 fields under a list head of their own: the payload without its last 42 bytes
 * (MixDigest and Nonce).  Both rows are zeros for a header with GSV_ST_BAD_RLP.
 *
 * Parent (verifyHeaderWorker).  For i > 0 the parent is header i - 1 when Hash(i - 1) == ParentHash(i), whatever
 * header i - 1's own status; else GSV_ST_UNKNOWN_ANCESTOR.  OURS: a header behind one that did not decode (BAD_RLP
 * or HEADER_TOO_WIDE) is GSV_ST_UNKNOWN_ANCESTOR, since the reference never holds such a header in its slice.  For
 * i = 0 the caller's parent_rlp (parent_len == 0: none) stands for chain.GetHeader(ParentHash, Number - 1): it is
 * the parent when it decodes, its Hash() is ParentHash(0) and its Number is Number(0) - 1 in uint64; else
 * GSV_ST_UNKNOWN_ANCESTOR.  The "known block" short cut (consensus.go:162-164) is a lookup in the caller's
 * database and is NOT here: a caller who wants it drops the known headers' statuses.
 *
 * Checks, in verifyHeader's order; the first failure is the status:
 *    1. len(Extra) > 32                                                  GSV_ST_EXTRA_TOO_LONG
 *    2. Time > now + 15                                                  GSV_ST_FUTURE_BLOCK
 *    3. Time <= parent.Time                                              GSV_ST_ZERO_BLOCK_TIME
 *    4. CalcDifficulty(config, Time, parent) != Difficulty               GSV_ST_WRONG_DIFFICULTY
 *    5. GasLimit > 2^63 - 1                                              GSV_ST_GAS_LIMIT_CAP
 *    6. GasUsed > GasLimit                                               GSV_ST_GAS_USED
 *    7. |int64(parent.GasLimit) - int64(GasLimit)| >= parent.GasLimit / 1024 or GasLimit < 5000
 *                                                                        GSV_ST_GAS_LIMIT_BOUNDS
 *       (the reference's two's-complement conversions: a parent above 2^63 wraps as int64() does)
 *    8. Number - parent.Number != 1                                      GSV_ST_INVALID_NUMBER
 *    9. where seals[i]: VerifySeal (the light form above)                GSV_ST_INVALID_DIFFICULTY / _MIX_DIGEST / _POW
 *   10. misc.VerifyDAOHeaderExtraData (consensus/misc/dao.go:47-69)      GSV_ST_BAD_PRO_DAO_EXTRA / GSV_ST_BAD_NO_DAO_EXTRA
 *   11. misc.VerifyForkHashes (consensus/misc/forks.go:30-43)            GSV_ST_FORK_HASH
 * CalcDifficulty (consensus.go:297-459): the Frontier, Homestead or Byzantium rule by parent.Number + 1 (which does
 * not wrap) against the configuration, in 256-bit arithmetic with a carry out.  An expected value of 2^256 or
 * more equals no header's difficulty: GSV_ST_WRONG_DIFFICULTY, and the expected-difficulty row is 32 bytes of 0xFF.
 *
 * gsv_chain_config: the fields of params.ChainConfig (params/config.go:103-124) these rules read.  has_* is the
 * big.Int pointer being non-nil.  `reserved` is zero. */
typedef struct gsv_chain_config {
    uint64_t homestead_block; /* HomesteadBlock */
    uint64_t dao_fork_block;  /* DAOForkBlock */
    uint64_t eip150_block;    /* EIP150Block */
    uint64_t byzantium_block; /* ByzantiumBlock */
    uint8_t has_homestead, has_dao_fork, has_eip150, has_byzantium;
    uint8_t dao_fork_support; /* DAOForkSupport */
    uint8_t reserved[3];
    uint8_t eip150_hash[32]; /* EIP150Hash; all zero: not checked (misc/forks.go:37) */
} gsv_chain_config;
/* Host forms.  They stage, run and copy back; n == 0: success, nothing enqueued.
 *   hash:       hash32 / hash_no_nonce32 (either may be NULL) row i, status[i] the decode status (GSV_ST_OK,
 *               GSV_ST_BAD_RLP, GSV_ST_HEADER_TOO_WIDE).
 *   difficulty: difficulty32 row i = CalcDifficulty(config, time[i], parent i) as 32 big-endian bytes, parent i =
 *               parent_rlp[parent_off[i] .. parent_off[i+1]); status[i] the parent's decode status (row of zeros),
 *               or GSV_ST_WRONG_DIFFICULTY with a row of 0xFF for a value of 2^256 or more.  time[i] may lie
 *               before the parent's time (big.Int.Div floors).
 *   headers:    the whole of VerifyHeaders.  seals: n bytes, NULL = all true.  now: Unix seconds, at most 2^63
 *               (else GSV_E_INVALID_ARG).  test_mode as in the seal forms.  hash32 (NULL or n rows): Hash() of each
 *               header.  expected_difficulty32 (NULL or n rows): what check 4 compared against, zeros for a header
 *               that failed before it.  The flow: decode and rules on the device; Number and the pre-seal status
 *               come back; the headers with seals[i] that have passed so far (the reference never runs VerifySeal
 *               behind an earlier failure) are grouped by epoch through the context's cache list and run through the
 *               light kernel, as gsv_ethash_verify_seal_batch does; the three statuses are merged on the device. */
int gsv_block_header_hash_batch(gsv_ctx *ctx, const uint8_t *rlp, const uint64_t *off, size_t n, uint8_t *hash32,
                                uint8_t *hash_no_nonce32, uint8_t *status);
int gsv_calc_difficulty_batch(gsv_ctx *ctx, const gsv_chain_config *config, const uint64_t *time,
                              const uint8_t *parent_rlp, const uint64_t *parent_off, size_t n, uint8_t *difficulty32,
                              uint8_t *status);
int gsv_ethash_verify_headers_batch(gsv_ctx *ctx, const gsv_chain_config *config, const uint8_t *rlp,
                                    const uint64_t *off, size_t n, const uint8_t *parent_rlp, size_t parent_len,
                                    const uint8_t *seals, uint64_t now, int test_mode, uint8_t *status, uint8_t *hash32,
                                    uint8_t *expected_difficulty32);
/* Device-resident forms.  Both only enqueue on `stream` (NULL = the context stream): no allocation, no
 * synchronisation, no prepare call (the configuration and `now` travel as kernel arguments), capturable; n == 0:
 * success, nothing enqueued.  The caller runs gsv_ethash_verify_seal_batch_dev between them over one epoch's cache.
 *   rules: two launches, k_block_header (GSV_K_BLOCK_HEADER) and k_block_header_rules (GSV_K_BLOCK_RULES).  d_rlp and
 *          d_off as in gsv_keccak256_batch_dev; d_parent_rlp parent_len bytes in HBM (parent_len == 0: no parent,
 *          the pointer is not read).  d_work: gsv_block_header_work_bytes(n) bytes of the caller's, 16-byte
 *          aligned: the records the two launches hand each other.  It writes the four arrays the seal call takes:
 *          d_hash_no_nonce32 (4-byte aligned), d_nonce (8-byte aligned; Header.Nonce.Uint64()), d_mix32 and
 *          d_difficulty32 (any alignment), zeros for a header that did not decode; d_pre_status and
 *          d_post_status (checks 1-8 and the link; checks 10-11); and, each NULL or n rows, d_hash32 (any
 *          alignment), d_number (8-byte aligned) and d_expected_difficulty32 (any alignment).  The kernels read no
 *          byte outside d_rlp[d_off[0] .. d_off[n]) and the parent but for the other bytes of the aligned dwords
 *          that hold an item's first and last byte.
 *   merge: one launch (GSV_K_BLOCK_MERGE).  d_status[i] = d_pre_status[i] if it is not GSV_ST_OK; else
 *          d_seal_status[i] where d_seal_status is not NULL and d_seals is NULL or d_seals[i] != 0, if it is not
 *          GSV_ST_OK; else d_post_status[i].
 * GSV_E_INVALID_ARG: a NULL context, configuration or required array, a misaligned array, now above 2^63, n or
 * parent_len above 2^31 - 1. */
size_t gsv_block_header_work_bytes(size_t n);
int gsv_block_header_rules_dev(gsv_ctx *ctx, const gsv_chain_config *config, const uint8_t *d_rlp,
                               const uint64_t *d_off, size_t n, const uint8_t *d_parent_rlp, size_t parent_len,
                               uint64_t now, uint8_t *d_work, uint8_t *d_hash_no_nonce32, uint64_t *d_nonce,
                               uint8_t *d_mix32, uint8_t *d_difficulty32, uint8_t *d_pre_status, uint8_t *d_post_status,
                               uint8_t *d_hash32, uint64_t *d_number, uint8_t *d_expected_difficulty32, void *stream);
int gsv_block_header_merge_dev(gsv_ctx *ctx, const uint8_t *d_pre_status, const uint8_t *d_seal_status,
                               const uint8_t *d_seals, const uint8_t *d_post_status, size_t n, uint8_t *d_status,
                               void *stream);

/* ---- clique: the voting snapshot and the fold of Clique.VerifyHeaders (consensus/clique), host only ----
 * The part of Clique.VerifyHeaders that is serial by nature runs here, on the host, over one RECORD per header that
 * the caller packs from what is computed per header in parallel: Hash(), the signer (gsv_ecrecover_batch over sigHash,
 * clique.go:146-168, and Extra[len - 65 :], :171-193) and the STATIC status, the checks of verifyHeader and
 * verifyCascadingFields that need no snapshot, in the reference's order, first failure wins:
 *    0. decode                                                             GSV_ST_BAD_RLP / GSV_ST_HEADER_TOO_WIDE
 *    1. Time > now (full width; :275; no + 15 here)                        GSV_ST_FUTURE_BLOCK
 *    2. checkpoint (Number % Epoch == 0) and Coinbase != 0 (:280)          GSV_ST_CLIQUE_CHECKPOINT_BENEFICIARY
 *    3. Nonce neither ff..ff nor 00..00 (:284)                             GSV_ST_CLIQUE_INVALID_VOTE
 *    4. checkpoint and Nonce != 0 (:287)                                   GSV_ST_CLIQUE_CHECKPOINT_VOTE
 *    5. len(Extra) < 32 (:291)                                             GSV_ST_CLIQUE_MISSING_VANITY
 *    6. len(Extra) < 97 (:294)                                             GSV_ST_CLIQUE_MISSING_SIGNATURE
 *    7. not checkpoint and len(Extra) != 97 (:299)                         GSV_ST_CLIQUE_EXTRA_SIGNERS
 *    8. checkpoint and (len(Extra) - 97) % 20 != 0 (:302)                  GSV_ST_CLIQUE_CHECKPOINT_SIGNERS
 *    9. MixDigest != 0 (:306)                                              GSV_ST_CLIQUE_MIX_DIGEST
 *   10. UncleHash != EmptyUncleHash (:310)                                 GSV_ST_CLIQUE_UNCLE_HASH
 *   11. Number > 0 and Difficulty not 1 or 2 (:314)                        GSV_ST_CLIQUE_DIFFICULTY
 *   12. misc.VerifyForkHashes (:320; clique has no DAO extra-data check)   GSV_ST_FORK_HASH
 *   13. Number > 0: the parent in front decoded, its Number is Number - 1 (uint64) and its Hash() is ParentHash
 *       (:344); else                                                       GSV_ST_UNKNOWN_ANCESTOR
 *   14. Number > 0: parent.Time.Uint64() + Period > Time.Uint64(), in wrapping uint64 arithmetic on the low 64
 *       bits as Go's (:347)                                                GSV_ST_CLIQUE_INVALID_TIMESTAMP
 * The library has no device form of these per-header steps yet: the record is the contract such a form is to meet.
 * A record is 128 bytes (csrc/clique_host.h):
 *   hash 32 | parent_hash 32 | signer 20 | coinbase 20 | number 8 (little-endian) | extra_off 4 | extra_len 4 |
 *   static status 1 | signer status 1 | vote 1 | difficulty 1 | zero 4
 * extra_off is the offset of Extra's first byte from the header's first byte and extra_len its FULL length; the
 * signer status is GSV_ST_OK, GSV_ST_INVALID_RECID, GSV_ST_RECOVER_FAILED, or GSV_ST_CLIQUE_MISSING_SIGNATURE when
 * len(Extra) < 65; vote is 0 (Nonce 00..00, drop), 1 (ff..ff, authorize) or 2 (neither); difficulty is 1, 2, or 0
 * for anything else; number is 0 for a header that did not decode or whose Number is wider than 8 bytes.
 *
 * The snapshot (snapshot.go:46-57) is an opaque gsv_clique_snapshot on the host: Number, Hash, Signers, Recents,
 * Votes in order, Tally.  These calls need no device and no context.
 *   new:          the snapshot at block `number` with hash `hash32` over n signers (newSnapshot, :62-76); NULL on a
 *                 NULL hash or signer array
 *   from_genesis: the snapshot at block 0 from an RLP-encoded genesis header: the signer list is Extra[32 : len - 65],
 *                 (len - 97) / 20 addresses (clique.go:397-401), the hash the header's.  NULL and *status (NULL ok) =
 *                 GSV_ST_BAD_RLP, GSV_ST_CLIQUE_MISSING_VANITY or GSV_ST_CLIQUE_MISSING_SIGNATURE otherwise
 *   copy, free:   a deep copy (:104-127); free(NULL) is fine
 *   number, hash: the block the snapshot stands at
 *   signers:      ascending (snapshot.go:288-301); recents: by ascending block; votes: chronological; tally: by
 *                 ascending address.  Each returns the count and fills at most `cap` entries of the arrays that are
 *                 not NULL (signer20 / address20 rows of 20 bytes, block uint64, authorize uint8, votes int32)
 *   inturn:       Snapshot.inturn (:304-310), 0 for an empty signer set (the reference divides by zero)
 *   gsv_clique_calc_difficulty: CalcDifficulty(snap, signer) (clique.go:669-676): 2 in turn at snap.Number + 1, else 1
 *
 * gsv_clique_fold(snap, config, records, n, rlp, off, status, applied): verifyCascadingFields' snapshot half, verifySeal
 * and Snapshot.apply over the records of n consecutive headers.  snap is at the parent of header 0 and is moved to
 * the last header applied.  rlp / off are the caller's headers on the HOST (read only for a checkpoint's signer list,
 * at the record's offsets).  With a sticky error err = GSV_ST_OK, status[i] is
 *   1. the static status if it is not GSV_ST_OK;
 *   2. else GSV_ST_OK if Number == 0 (verifyCascadingFields returns nil, clique.go:334), and nothing is applied;
 *   3. else err if it is not GSV_ST_OK (snapshot() failed on an earlier header, :351-354);
 *   4. else for a checkpoint: GSV_ST_CLIQUE_CHECKPOINT_SIGNERS if Extra[32 : len - 65] is not the snapshot's sorted
 *      signers (:356-365);
 *   5. else verifySeal (:478-502): the signer status; the signer not in Signers: GSV_ST_CLIQUE_UNAUTHORIZED; a recent
 *      signer with seen > number - limit (limit = len(Signers) / 2 + 1, uint64): GSV_ST_CLIQUE_UNAUTHORIZED; the turn
 *      rule against Difficulty (in turn 2, else 1): GSV_ST_CLIQUE_DIFFICULTY.
 * Then header i is applied exactly as Snapshot.apply does (snapshot.go:192-280), WHATEVER status[i] was (the reference
 * applies a parent that failed verifyHeader, too): the epoch reset, the oldest recent dropped, the signer status,
 * unauthorized, recent, the previous vote uncast, the nonce read as a vote (GSV_ST_CLIQUE_INVALID_VOTE), cast,
 * majority, the signer added or dropped with the second recents delete, votes by and about the account discarded.
 * GSV_ST_CLIQUE_VOTING_CHAIN when Number != snap.Number + 1 (:181-188).  A failing apply sets err, leaves the snapshot
 * at the last header applied and stops the count in *applied (NULL ok).
 * OURS, not the reference's: a header that did not decode, or whose ParentHash is not the snapshot's Hash (for header
 * 0: the caller's snapshot is not at its parent), sets err = GSV_ST_UNKNOWN_ANCESTOR.  The reference would walk to its
 * database for the missing ancestors (clique.go:408-425), which the call does not have.
 * GSV_E_INVALID_ARG: a NULL snapshot, configuration, record or status array, rlp or off NULL with n > 0, epoch == 0. */
typedef struct gsv_clique_config {
    uint64_t period; /* params.CliqueConfig.Period */
    uint64_t epoch;  /* params.CliqueConfig.Epoch; 0 is GSV_E_INVALID_ARG (clique.New defaults it to 30000: the caller's) */
} gsv_clique_config;
typedef struct gsv_clique_snapshot gsv_clique_snapshot;
gsv_clique_snapshot *gsv_clique_snapshot_new(const uint8_t *signers20, size_t n, uint64_t number, const uint8_t *hash32);
gsv_clique_snapshot *gsv_clique_snapshot_from_genesis(const uint8_t *header_rlp, size_t len, int *status);
gsv_clique_snapshot *gsv_clique_snapshot_copy(const gsv_clique_snapshot *snap);
void gsv_clique_snapshot_free(gsv_clique_snapshot *snap);
uint64_t gsv_clique_snapshot_number(const gsv_clique_snapshot *snap);
int gsv_clique_snapshot_hash(const gsv_clique_snapshot *snap, uint8_t *hash32);
size_t gsv_clique_snapshot_signers(const gsv_clique_snapshot *snap, uint8_t *signer20, size_t cap);
size_t gsv_clique_snapshot_recents(const gsv_clique_snapshot *snap, uint64_t *block, uint8_t *signer20, size_t cap);
size_t gsv_clique_snapshot_votes(const gsv_clique_snapshot *snap, uint8_t *signer20, uint64_t *block,
                                 uint8_t *address20, uint8_t *authorize, size_t cap);
size_t gsv_clique_snapshot_tally(const gsv_clique_snapshot *snap, uint8_t *address20, uint8_t *authorize,
                                 int32_t *votes, size_t cap);
int gsv_clique_snapshot_inturn(const gsv_clique_snapshot *snap, uint64_t number, const uint8_t *signer20);
int gsv_clique_calc_difficulty(const gsv_clique_snapshot *snap, const uint8_t *signer20);
int gsv_clique_fold(gsv_clique_snapshot *snap, const gsv_clique_config *config, const uint8_t *records, size_t n,
                    const uint8_t *rlp, const uint64_t *off, uint8_t *status, size_t *applied);
/* ---- synthetic signed workload (bench / test data generator; signing is not on the path) ----
 * key_i, msg_i, nonce_i = Keccak256(le64(seed) || le64(i) || "key"/"msg"/"nce"), key and nonce
 * reduced mod n (0 -> 1); sig_i = ECDSA(key_i, msg_i, nonce_i), low-s normalised, recid in sig[64].
 * pub65/addr20 (optional) receive the signer's key and address (the expected recovery result). */
int gsv_synth_sign(gsv_ctx *ctx, uint64_t seed, size_t n, uint8_t *msg32, uint8_t *sig65,
                   uint8_t *pub65, uint8_t *addr20);
int gsv_synth_sign_dev(gsv_ctx *ctx, uint64_t seed, size_t n, uint8_t *d_msg32, uint8_t *d_sig65,
                       uint8_t *d_pub65, uint8_t *d_addr20, void *stream);

/* ---- synthetic pairing workload (bench / test data; configs[4]) ----
 * nchecks x 768 B precompile inputs: check i = e(aP,bQ) e(-bP,aQ) e(cP,dQ) e(-dP,cQ) (true) with
 * a..d = Keccak256(le64(seed) || le64(i) || tag) mod 2^253; i % 8 == 7 perturbs d (false);
 * i % 1024 == 1023 also sets a coordinate to p (bad input).  expect (optional) gets the verdicts. */
int gsv_bn256_synth_checks_dev(gsv_ctx *ctx, uint64_t seed, size_t nchecks, uint8_t *d_out768,
                               uint8_t *d_expect, void *stream);

/* ---- notary validation of whole collations (configs[3]) ----
 * Shard s body = bodies[off[s] .. off[s+1]), at most 2^20 bytes (sharding/collation.go:45).  On the
 * GPU: blob-deserialize (sharding/utils/marshal.go:144-198), decode every blob as an RLP transaction
 * and recover its sender with the signer (GSV_SIGNER_*, chain_id big-endian; the reference notary's
 * chain uses EIP-155), and compute the chunk root (sharding/collation.go:115-119).
 * Per shard: root32_out[32], ntx_out = number of blobs, valid_bitmap_out[(max_txs+7)/8] with bit t
 * (LSB first) set when tx t's sender recovered (GSV_ST_OK).  Optional per tx, laid out
 * [n_shards][max_txs]: senders_out (20 B, zero when not OK) and status_out (GSV_ST_*).
 * A shard with more than max_txs blobs: only the first max_txs are validated; the host entry point
 * returns GSV_E_TOO_LARGE for it (the _dev one reports it through ntx > max_txs).
 * 1 <= max_txs <= GSV_MAX_TXS_PER_SHARD (every blob takes at least one 32-byte chunk of a body of at
 * most 2^20 bytes), else GSV_E_INVALID_ARG; at most 65,535 shards per call. */
#define GSV_MAX_TXS_PER_SHARD 32768
int gsv_notary_validate_shards(gsv_ctx *ctx, const uint8_t *bodies, const uint64_t *off, size_t n_shards,
                               const uint8_t *chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs,
                               uint8_t *root32_out, uint32_t *ntx_out, uint8_t *valid_bitmap_out,
                               uint8_t *senders_out, uint8_t *status_out);
/* Device-resident form: d_bodies/outputs in HBM, h_off on the host; enqueues on `stream`.
 * gsv_notary_prepare prepares it for exactly (h_off, chain id, signer_kind, max_txs). */
int gsv_notary_prepare(gsv_ctx *ctx, const uint64_t *h_off, size_t n_shards, const uint8_t *chain_id,
                       size_t chain_id_len, int signer_kind, uint32_t max_txs);
int gsv_notary_validate_shards_dev(gsv_ctx *ctx, const uint8_t *d_bodies, const uint64_t *h_off, size_t n_shards,
                                   const uint8_t *chain_id, size_t chain_id_len, int signer_kind,
                                   uint32_t max_txs, uint8_t *d_root32, uint32_t *d_ntx, uint8_t *d_bitmap,
                                   uint8_t *d_senders, uint8_t *d_status, void *stream);

/* ---- synthetic collations (bench / test data; configs[3]) ----
 * Bodies of shards shard0 .. shard0+n_shards-1 (txs_per_shard x 128 B each, contiguous): signed
 * EIP-155 txs (chain id 1) blob-serialized 4 chunks per tx; every 128th tx invalid by construction
 * (high-s / wrong chain id / r not an x-coordinate / recid flipped).  Optional expected status and
 * sender per tx; exp_sender holds the SIGNER's address, which a recid-flipped tx (status OK) does not
 * recover to. */
int gsv_notary_synth_dev(gsv_ctx *ctx, uint64_t seed, uint32_t shard0, size_t n_shards, uint32_t txs_per_shard,
                         uint8_t *d_bodies, uint8_t *d_exp_status, uint8_t *d_exp_sender, void *stream);

/* ---- DeriveSha over any DerivableList (tx root, receipt root) ----
 * List i holds items [list_off[i], list_off[i+1]) of the global item array; item k =
 * vals[voff[k] .. voff[k+1]) is list.GetRlp(j) — the RLP the reference inserts under key rlp(j)
 * (core/types/derive_sha.go:36-38; rlp(tx) for Transactions, rlp(receipt) for Receipts).
 * root32_out[i] = DeriveSha(list i); an empty list gives emptyRoot.  Lists of up to 2^24 items. */
int gsv_derive_sha_batch(gsv_ctx *ctx, const uint8_t *vals, const uint64_t *voff, const uint64_t *list_off,
                         size_t n_lists, uint8_t *root32_out);
/* Device-resident form: d_vals in HBM; voff / list_off on the host (offsets into d_vals / item
 * indices); d_root32_out in HBM; enqueues on `stream` (NULL = the context stream).
 * gsv_derive_sha_prepare prepares it for exactly (voff, list_off). */
int gsv_derive_sha_prepare(gsv_ctx *ctx, const uint64_t *voff, const uint64_t *list_off, size_t n_lists);
int gsv_derive_sha_batch_dev(gsv_ctx *ctx, const uint8_t *d_vals, const uint64_t *voff, const uint64_t *list_off,
                             size_t n_lists, uint8_t *d_root32_out, void *stream);

/* ---- logs bloom and receipts: the receipt half of BlockValidator.ValidateState (core/block_validator.go:80-95) ----
 * bloom9 (core/types/bloom9.go:115-127): Keccak-256 of a byte string; its three bits are the low 11 bits of the
 * big-endian byte pairs 0-1, 2-3 and 4-5 of the digest.  Bit b of a 2,048-bit Bloom lies in byte 255 - b / 8 under
 * mask 1 << (b % 8) (the big.Int layout, core/bloombits/generator.go:64-70).
 *   gsv_bloom9_batch: message i = data[off[i] .. off[i+1]), any length; idx_out[3 i .. 3 i + 3) = its three bit
 *   numbers.  What BloomLookup and a bloombits filter test.  The _dev form takes device arrays (the n + 1 offsets
 *   included; d_idx_out 2-byte aligned) and only enqueues one launch (GSV_K_BLOOM9): no allocation, no
 *   synchronisation, no prepare call, capturable.  n == 0: success, nothing enqueued. */
int gsv_bloom9_batch(gsv_ctx *ctx, const uint8_t *data, const uint64_t *off, size_t n, uint16_t *idx_out);
int gsv_bloom9_batch_dev(gsv_ctx *ctx, const uint8_t *d_data, const uint64_t *d_off, size_t n, uint16_t *d_idx_out,
                         void *stream);
/* Receipts.  Receipt k = vals[voff[k] .. voff[k+1]) is Receipts.GetRlp(k), the consensus encoding
 * rlp([PostStateOrStatus, CumulativeGasUsed, Bloom, Logs]) (core/types/receipt.go:67-73, :98-100); list i (one
 * block) holds receipts [list_off[i], list_off[i+1]), as gsv_derive_sha_batch takes its items.
 *
 * Decode, as rlp.DecodeBytes into types.Receipt (receipt.go:104-114, core/types/log.go:65-95): a list of exactly four
 * items; PostStateOrStatus a string; CumulativeGasUsed a uint64 (no leading zero byte, at most 8 bytes); Bloom of
 * exactly 256 bytes; Logs a list of lists of exactly three items: Address of exactly 20 bytes, Topics a list of any
 * number of 32-byte strings (the decoder has no cap of four), Data a string.  Every length in its shortest form, a
 * single byte below 0x80 as itself, no element missing or left over, no length past its list or the input, no byte
 * behind the list, no empty input.  What the reference's decoder refuses is GSV_ST_BAD_RLP.  A receipt that
 * decodes and whose status field is none of the empty string, the byte 01 or 32 bytes is GSV_ST_RECEIPT_STATUS
 * (setStatus, receipt.go:116-128); as in the reference, that is judged before bytes behind the list are.  The
 * Bloom field of a receipt is carried, not checked: ValidateState compares the block's bloom only.
 *
 * Bloom.  LogsBloom (bloom9.go:103-113) ORs bloom9 of each log's Address and of each of its Topics; CreateBloom
 * (:94-101) ORs that over a list's receipts.  The decoder accepts canonical encodings only, so a receipt that
 * decodes re-encodes to the same bytes, and the receipt root is gsv_derive_sha_batch over the very same vals.
 *
 * Per list, in this order; the first that applies is the status:
 *    1. the status of the first receipt of the list that is not GSV_ST_OK.  OURS: the reference never gets as
 *       far as ValidateState with a receipt that does not decode.  Such a list has a zero bloom row, a zero root
 *       row and gas used 0.
 *    2. gas used != want_gas_used[i]                     GSV_ST_GAS_USED_MISMATCH   (block_validator.go:82-84)
 *    3. bloom row != want_bloom256 row i                 GSV_ST_INVALID_BLOOM       (:87-90)
 *    4. receipt root != want_root32 row i                GSV_ST_INVALID_RECEIPT_ROOT (:92-95)
 *    5. else                                             GSV_ST_OK
 * Gas used is the last receipt's CumulativeGasUsed, 0 for an empty list (an empty list has a zero bloom and
 * emptyRoot).  The state root (IntermediateRoot, :98-100) needs the state database and stays with the caller.
 *
 * Host form.  gsv_receipts_verify_batch stages, runs the chain below with DeriveSha in the middle and copies back.
 * Each want_* may be NULL: that compare is skipped, so with all three NULL the call is CreateBloom plus the
 * receipt root.  Outputs, each NULL or its full size: receipt_status (one byte per receipt of
 * [list_off[0], list_off[n_lists])), list_bloom256 (n_lists x 256), root32 (n_lists x 32), gas_used (n_lists);
 * status (n_lists bytes) is required.  n_lists == 0: success, nothing launched.  GSV_E_INVALID_ARG before any HIP
 * call: a NULL context, table or status, a table that steps backwards, 2^31 receipts or more; GSV_E_TOO_LARGE: a
 * receipt of 2^32 bytes or more, or more than 2^40 bytes of receipts.
 *
 * Device-resident forms.  Both only enqueue on `stream` (NULL = the context stream): no allocation, no
 * synchronisation, no prepare call, capturable.  The caller runs gsv_derive_sha_batch_dev between them.
 *   bloom: memset nodes over the work area's descriptor table and the bloom rows, then three launches:
 *          k_receipt_scan (GSV_K_RECEIPT_SCAN), k_receipt_bloom (GSV_K_RECEIPT_BLOOM: one lane per bloom ITEM, so
 *          a receipt of hundreds of logs costs what its items cost) and k_receipt_lists (GSV_K_RECEIPT_LISTS).
 *          d_voff: n_receipts + 1 ascending offsets into d_vals, in HBM; d_voff[0] may be nonzero and d_vals may
 *          have any alignment.  d_list_off: n_lists + 1 ascending receipt indices in [0, n_receipts], in HBM; a
 *          receipt no list holds is decoded and joins no row.  Both tables 8-byte aligned.  vals_bytes: the
 *          caller's bound on d_voff[n_receipts] - d_voff[0], at most 2^40.  OURS: a receipt that reaches past
 *          vals_bytes (or starts before d_voff[0], or ends before it starts, or is 2^32 bytes or longer) is
 *          GSV_ST_BAD_RLP unread, and no byte outside d_work is ever written for it.  d_work:
 *          gsv_receipts_work_bytes(n_receipts, vals_bytes) bytes of the caller's, 8-byte aligned (0: past the
 *          bounds).  Writes d_receipt_status (n_receipts), d_receipt_bloom256 (n_receipts x 256, may be NULL),
 *          d_list_bloom256 (n_lists x 256), d_gas_used (n_lists, 8-byte aligned), d_list_status (n_lists: rule 1
 *          alone).  Byte outputs have any alignment: the bloom rows are written by dword atomics on the aligned
 *          dwords that hold their bytes, which OR zeros into the up to three bytes in front of and behind them.
 *          The kernels read no byte outside d_vals[d_voff[0] .. d_voff[0] + vals_bytes) but for the other bytes
 *          of the aligned dwords that hold an item's first and last byte.
 *   check: one launch (GSV_K_RECEIPT_CHECK): rules 1-5 over d_list_status_in, d_list_bloom256, d_root32 and
 *          d_gas_used against the d_want_* arrays (each may be NULL; d_want_gas_used 8-byte aligned).  d_root32 is
 *          read and, for a list under rule 1, overwritten with zeros.
 * GSV_E_INVALID_ARG: a NULL context or required array, a misaligned table, d_work or gas array, n_receipts or
 * n_lists above 2^31 - 1, vals_bytes above 2^40.  n_lists == 0: success, nothing enqueued. */
size_t gsv_receipts_work_bytes(size_t n_receipts, uint64_t vals_bytes);
int gsv_receipts_bloom_dev(gsv_ctx *ctx, const uint8_t *d_vals, const uint64_t *d_voff, size_t n_receipts,
                           const uint64_t *d_list_off, size_t n_lists, uint64_t vals_bytes, uint8_t *d_work,
                           uint8_t *d_receipt_status, uint8_t *d_receipt_bloom256, uint8_t *d_list_bloom256,
                           uint64_t *d_gas_used, uint8_t *d_list_status, void *stream);
int gsv_receipts_check_dev(gsv_ctx *ctx, const uint8_t *d_list_status_in, const uint8_t *d_list_bloom256,
                           uint8_t *d_root32, const uint64_t *d_gas_used, const uint8_t *d_want_bloom256,
                           const uint8_t *d_want_root32, const uint64_t *d_want_gas_used, size_t n_lists,
                           uint8_t *d_status, void *stream);
int gsv_receipts_verify_batch(gsv_ctx *ctx, const uint8_t *vals, const uint64_t *voff, const uint64_t *list_off,
                              size_t n_lists, const uint8_t *want_bloom256, const uint8_t *want_root32,
                              const uint64_t *want_gas_used, uint8_t *receipt_status, uint8_t *list_bloom256,
                              uint8_t *root32, uint64_t *gas_used, uint8_t *status);

/* ---- bloombits: section generator, bitset codec, matcher, bloomFilter ----
 * Mirrors core/bloombits (generator.go, matcher.go), the codec of common/bitutil (compress.go) and bloomFilter
 * (eth/filters/filter.go:278-305).  Results are byte for byte the reference's.
 *
 * Numbering.  Bloom bit b (0 .. 2047) of a 256-byte bloom is byte 255 - b / 8 under mask 1 << (b % 8)
 * (generator.go:64-70): the numbers gsv_bloom9_batch returns.  A section of S blooms, S % 8 == 0 (:40), becomes
 * 2,048 bit vectors of S / 8 bytes; block j of the section is byte j / 8 of a vector under mask 1 << (7 - j % 8)
 * (:61-62).  The table of n_sections sections is dense: bits[(section * 2048 + bit) * (S / 8) + byte].
 * OURS: 8 <= S <= 32,768 (GSV_BLOOMBITS_MAX_SECTION; the reference's own benchmark stops there,
 * eth/filters/bench_test.go:60) and S % 8 == 0; anything else is GSV_E_INVALID_ARG.  OURS: at most 2^20 sections and
 * 2^20 queries, rules and clauses a call, and at most 2^24 (query, section) pairs.
 *
 * Every _dev form takes device arrays and only enqueues on `stream` (NULL = the context stream): no allocation, no
 * synchronisation, no prepare call, capturable.  A NULL context or required array, a misaligned table of offsets
 * or counts, or a size past the bounds above is GSV_E_INVALID_ARG before any HIP call.  A call over no items
 * (n_sections, n, n_queries or n_blooms of 0) is success and enqueues nothing.
 *
 * 1. Generator (generator.go:52-87: AddBloom over a whole section, then every Bitset).  blooms: n_sections x S rows
 *    of 256 bytes, any alignment; bits: the table above, any alignment.  One launch (GSV_K_BLOOMBITS_GENERATE). */
#define GSV_BLOOMBITS_MAX_SECTION 32768
#define GSV_BLOOM_BITS 2048
int gsv_bloombits_generate_batch(gsv_ctx *ctx, const uint8_t *blooms256, size_t n_sections, uint32_t section_size,
                                 uint8_t *bits_out);
int gsv_bloombits_generate_dev(gsv_ctx *ctx, const uint8_t *d_blooms256, size_t n_sections, uint32_t section_size,
                               uint8_t *d_bits, void *stream);
/* 2. Codec over n vectors of one length L each, 1 <= L <= GSV_BITSET_MAX_LEN, n < 2^31.
 *    Compress = CompressBytes (compress.go:60-67) around bitsetEncodeBytes (:71-97): vector i = d_in[i L .. i L + L);
 *    its result lies in slot i = d_slots[i L ..) with d_len[i] (4-byte aligned) bytes: 0 = all zero (:93-95, :78-80),
 *    L = stored raw (:61-66: the encoding was not shorter), else the recursive encoding.  The encoding of a dense
 *    vector is longer than L, so the kernel settles the length before it writes: no byte of a slot behind d_len[i]
 *    and no byte outside the slots is written.  One launch (GSV_K_BITSET_COMPRESS).  The host form returns the
 *    packed concatenation: out_off[n + 1] (out_off[0] = 0) and out, which must hold n * L bytes.
 *    Decompress = DecompressBytes(data, L) (:102-112): input i = d_data[d_off[i] .. d_off[i + 1]) (n + 1 offsets,
 *    8-byte aligned, any start), output row i = d_out[i L ..), d_status[i]: GSV_ST_OK or the FIRST error the
 *    reference's recursion meets: a longer input than L is GSV_ST_BITSET_EXCEEDED_TARGET (:103-105), one of L bytes
 *    is copied (:106-110); else bitsetDecodePartialBytes (:130-170) innermost level first (:148-151), inside a level
 *    per set bit in order: GSV_ST_BITSET_MISSING_DATA (:155-157), GSV_ST_BITSET_EXCEEDED_TARGET (:158-160),
 *    GSV_ST_BITSET_ZERO_CONTENT (:162-164); last GSV_ST_BITSET_UNREFERENCED_DATA (:120-122).  OURS: an entry of the
 *    table that steps backwards is GSV_ST_BITSET_MISSING_DATA unread.  A failed vector's output row is zero.  One
 *    launch (GSV_K_BITSET_DECOMPRESS).  The host form checks its table (ascending, else GSV_E_INVALID_ARG). */
#define GSV_BITSET_MAX_LEN 4096
int gsv_bitset_compress_batch(gsv_ctx *ctx, const uint8_t *in, size_t n, uint32_t len, uint8_t *out,
                              uint64_t *out_off);
int gsv_bitset_compress_batch_dev(gsv_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t len, uint8_t *d_slots,
                                  uint32_t *d_len, void *stream);
int gsv_bitset_decompress_batch(gsv_ctx *ctx, const uint8_t *data, const uint64_t *off, size_t n, uint32_t len,
                                uint8_t *out, uint8_t *status);
int gsv_bitset_decompress_batch_dev(gsv_ctx *ctx, const uint8_t *d_data, const uint64_t *d_off, size_t n, uint32_t len,
                                    uint8_t *d_out, uint8_t *d_status, void *stream);
/* 3. Matcher.  The filter system of many queries over one table, as NewMatcher leaves it in Matcher.filters
 *    (matcher.go:105-122): query q holds rules [d_query_off[q], d_query_off[q + 1]), rule r holds clauses
 *    [d_rule_off[r], d_rule_off[r + 1]) (both uint32, 4-byte aligned, n_queries + 1 and n_rules + 1 entries), clause c
 *    is the three uint16 bit numbers d_clauses[3 c ..) (2-byte aligned), each masked to 11 bits: the layout
 *    gsv_bloom9_batch_dev writes.  An entry past n_rules / n_clauses is clamped to it, so no table is read past its
 *    end.  d_begin / d_end (8-byte aligned): the query's block range, both ends included (matcher.go:147, :182-192).
 *    d_bits holds sections [first_section, first_section + n_sections) of section_size blocks.
 *    Per query and section: all ones (matcher.go:238); per rule the OR over its clauses of the AND of the clause's
 *    three rows (:337-359), ANDed over the rules (:364-366); then the blocks outside [begin, end] cleared (:182-192).
 *    A query with no rules matches every block of its range (TestWildcardMatcher); a rule with no clauses matches
 *    none (:361-363; NewMatcher drops such a rule, and so do the host forms).  OURS: blocks outside the table are not
 *    reported (the reference would wait for a retrieval).
 *    match:  one launch (GSV_K_BLOOMBITS_MATCH).  d_match: n_queries x n_sections x S / 8 bytes, any alignment;
 *            d_count (4-byte aligned): the set bits of each (query, section).
 *    blocks: three launches (GSV_K_BLOOMBITS_TOTALS, _SCAN, _BLOCKS).  d_block_off (8-byte aligned, n_queries + 1):
 *            the scan of the queries' totals, d_block_off[0] = 0; query q's block numbers, ascending, are
 *            d_blocks[d_block_off[q] .. d_block_off[q + 1]) (8-byte aligned, `capacity` entries).  A number whose
 *            place is at or past `capacity` is not written; d_block_off holds the true totals all the same, so the
 *            caller sees the shortfall and calls again.
 *    Host form: the filter as NewMatcher takes it.  Clause c = clause_data[clause_off[c] .. clause_off[c + 1]) with
 *    clause_nil[c] != 0 for a nil clause (an empty clause that is not nil is hashed, a nil one is not; clause_nil
 *    NULL = none is nil); rule_off / query_off as above but uint64 on the host.  It drops a rule with no clauses and
 *    a rule with a nil clause (matcher.go:105-122), runs gsv_bloom9_batch_dev over the clauses that remain, then
 *    match, then blocks.  block_off_out: n_queries + 1; blocks_out: `capacity` entries, filled as by blocks_dev. */
int gsv_bloombits_match_dev(gsv_ctx *ctx, const uint8_t *d_bits, uint32_t section_size, uint64_t first_section,
                            size_t n_sections, const uint16_t *d_clauses, size_t n_clauses, const uint32_t *d_rule_off,
                            size_t n_rules, const uint32_t *d_query_off, size_t n_queries, const uint64_t *d_begin,
                            const uint64_t *d_end, uint8_t *d_match, uint32_t *d_count, void *stream);
int gsv_bloombits_blocks_dev(gsv_ctx *ctx, const uint8_t *d_match, const uint32_t *d_count, uint32_t section_size,
                             uint64_t first_section, size_t n_sections, size_t n_queries, uint64_t *d_block_off,
                             uint64_t *d_blocks, uint64_t capacity, void *stream);
int gsv_bloombits_match_batch(gsv_ctx *ctx, const uint8_t *bits, uint32_t section_size, uint64_t first_section,
                              size_t n_sections, const uint8_t *clause_data, const uint64_t *clause_off,
                              const uint8_t *clause_nil, const uint64_t *rule_off, const uint64_t *query_off,
                              size_t n_queries, const uint64_t *begin, const uint64_t *end, uint64_t *block_off_out,
                              uint64_t *blocks_out, uint64_t capacity);
/* 4. bloomFilter (eth/filters/filter.go:278-305) over n_blooms blooms of 256 bytes (any alignment), the queries in
 *    the matcher's layout (their ranges play no part): d_out[q * n_blooms + k] = 1 when bloom k passes query q, else
 *    0.  The rule evaluation is the matcher's; the bit test reads a bloom byte (BloomLookup, core/types/bloom9.go:131-
 *    136) where the matcher reads a row.  One launch (GSV_K_BLOOM_FILTER).  The host form takes the filter as
 *    gsv_bloombits_match_batch does and drops the same rules: filters.New (:62-93) never makes a nil clause, and a
 *    rule without clauses is bloomFilter's wildcard (:293). */
int gsv_bloom_filter_dev(gsv_ctx *ctx, const uint8_t *d_blooms256, size_t n_blooms, const uint16_t *d_clauses,
                         size_t n_clauses, const uint32_t *d_rule_off, size_t n_rules, const uint32_t *d_query_off,
                         size_t n_queries, uint8_t *d_out, void *stream);
int gsv_bloom_filter_batch(gsv_ctx *ctx, const uint8_t *blooms256, size_t n_blooms, const uint8_t *clause_data,
                           const uint64_t *clause_off, const uint8_t *clause_nil, const uint64_t *rule_off,
                           const uint64_t *query_off, size_t n_queries, uint8_t *out);

/* ---- Proof of Custody (sharding/collation.go:124-136) ----
 * poc32_out[i] = DeriveSha(Chunks(salt||b0||salt||b1||...)) over body i = bodies[off[i] .. off[i+1])
 * (salt alone for an empty body).  The salted body may hold up to 2^26 bytes (GSV_E_TOO_LARGE). */
int gsv_collation_poc_batch(gsv_ctx *ctx, const uint8_t *bodies, const uint64_t *off, size_t n,
                            const uint8_t *salt, size_t salt_len, uint8_t *poc32_out);
int gsv_collation_poc_prepare(gsv_ctx *ctx, const uint64_t *h_off, size_t n, const uint8_t *salt, size_t salt_len);
int gsv_collation_poc_batch_dev(gsv_ctx *ctx, const uint8_t *d_bodies, const uint64_t *h_off, size_t n,
                                const uint8_t *salt, size_t salt_len, uint8_t *d_poc32_out, void *stream);

/* ---- collation header hash + proposer signature ----
 * Header i = collationHeaderData{ShardID, ChunkRoot, Period, ProposerAddress, ProposerSignature}
 * (sharding/collation.go:35-43): shard_id32 / period32 are 32-byte big-endian integers,
 * chunk_root32, proposer20, sig65 = [R || S || V] as crypto.Sign returns it (V in {0,1}).
 * nil_flags (optional, NULL = all set): bit 0 = ChunkRoot nil, bit 1 = ProposerAddress nil,
 * bit 2 = ProposerSignature nil/empty (each then RLP-encodes as 0x80, rlp/encode.go:545-581).
 * hash32_out (optional): CollationHeader.Hash() of the header as given (signature included).
 * signer20_out (optional): crypto.Ecrecover(Hash() with ProposerSignature empty — the hash the
 * proposer signs at sharding/proposer/proposer.go:83 — , sig) -> address, zero on failure.
 * status: GSV_ST_OK when the signer equals ProposerAddress, GSV_ST_PROPOSER_MISMATCH when not,
 * else the recovery status (GSV_ST_INVALID_RECID / GSV_ST_RECOVER_FAILED).  A header with nil bit 2
 * set is never recovered: crypto.Ecrecover on an empty signature returns ErrInvalidSignatureLen
 * (crypto/secp256k1/secp256.go:171-174), so its status is GSV_ST_INVALID_SIG_LEN and its signer zero
 * whatever its sig65 row holds; its hash32_out is the hash with the signature empty. */
int gsv_collation_header_verify_batch(gsv_ctx *ctx, const uint8_t *shard_id32, const uint8_t *chunk_root32,
                                      const uint8_t *period32, const uint8_t *proposer20, const uint8_t *sig65,
                                      const uint8_t *nil_flags, size_t n, uint8_t *hash32_out,
                                      uint8_t *signer20_out, uint8_t *status);
/* Device-resident form: every array in HBM (d_nil_flags / d_hash32_out / d_signer20_out may be NULL);
 * enqueues on `stream` (NULL = the context stream) and returns.  gsv_collation_header_prepare sizes
 * its workspace for batches of n headers. */
int gsv_collation_header_prepare(gsv_ctx *ctx, size_t n);
int gsv_collation_header_verify_batch_dev(gsv_ctx *ctx, const uint8_t *d_shard_id32, const uint8_t *d_chunk_root32,
                                          const uint8_t *d_period32, const uint8_t *d_proposer20,
                                          const uint8_t *d_sig65, const uint8_t *d_nil_flags, size_t n,
                                          uint8_t *d_hash32_out, uint8_t *d_signer20_out, uint8_t *d_status,
                                          void *stream);

/* ---- blob codec: utils.Serialize / utils.Deserialize (sharding/utils/marshal.go:71-198) ----
 * Serialize.  List i (one collation) holds blobs [list_off[i], list_off[i+1]) of the global blob array;
 * blob k = blobs[blob_off[k] .. blob_off[k+1]) with flag skip_evm[k] (skip_evm NULL: all false).  Body i is
 * the concatenation of each blob's ceil(len / 31) chunks of 32 bytes: a non-terminal chunk is 00 and 31
 * data bytes, the terminal chunk is tl | (skip_evm ? 0x80 : 0) with tl = len - 31 (chunks - 1), tl data
 * bytes and 31 - tl zero bytes.  A ZERO-LENGTH BLOB EMITS NOTHING (getNumChunks(0) = 0), as in the
 * reference: Deserialize never gives that blob back.  No size limit here (the 2^20 limit is
 * SerializeTxToBlob's: see the proposer below); blobs of less than 2^32 bytes, fewer than 2^31 chunks per
 * call (GSV_E_TOO_LARGE).  The bodies lie contiguous at body_off_out[0 .. n_lists], each a multiple of 32.
 * gsv_blob_serialized_size is host arithmetic alone (no context, no GPU): body_off_out[n_lists + 1]. */
int gsv_blob_serialized_size(const uint64_t *blob_off, const uint64_t *list_off, size_t n_lists,
                             uint64_t *body_off_out);
int gsv_blob_serialize_batch(gsv_ctx *ctx, const uint8_t *blobs, const uint64_t *blob_off, const uint8_t *skip_evm,
                             const uint64_t *list_off, size_t n_lists, uint8_t *bodies_out, uint64_t *body_off_out);
/* Device-resident form: d_blobs and d_skip_evm (may be NULL) in HBM, the offset tables on the host;
 * d_bodies_out (16-byte aligned, gsv_blob_serialized_size's layout) in HBM.  One launch on `stream`; no
 * byte outside d_blobs[blob_off[list_off[0]] .. blob_off[list_off[n_lists]]) is read.
 * gsv_blob_serialize_prepare builds the chunk tables for exactly (blob_off, list_off). */
int gsv_blob_serialize_prepare(gsv_ctx *ctx, const uint64_t *blob_off, const uint64_t *list_off, size_t n_lists);
int gsv_blob_serialize_batch_dev(gsv_ctx *ctx, const uint8_t *d_blobs, const uint64_t *blob_off,
                                 const uint8_t *d_skip_evm, const uint64_t *list_off, size_t n_lists,
                                 uint8_t *d_bodies_out, void *stream);
/* Deserialize.  Body i = bodies[off[i] .. off[i+1]), at most 2^20 bytes (GSV_E_TOO_LARGE), at most 65,535
 * bodies.  Only whole chunks count (a trailing partial chunk is ignored); a chunk whose indicator & 0x1F
 * is tl != 0 ends a blob of 31 (chunks - 1) + tl bytes, indicator bit 7 is its skip_evm flag and no other
 * indicator bit is read; chunks after the last terminal chunk are dropped.
 * Host form: the reference's list of byte strings.  nblobs_out[i] = blobs of body i; the blobs of all
 * bodies in order are data_out[blob_off_out[k] .. blob_off_out[k+1]) with flag skip_evm_out[k].  Size
 * blob_off_out for sum(floor(len_i / 32)) + 1 entries, skip_evm_out for that many less one, data_out for
 * 31 sum(floor(len_i / 32)) bytes. */
int gsv_blob_deserialize_batch(gsv_ctx *ctx, const uint8_t *bodies, const uint64_t *off, size_t n,
                               uint32_t *nblobs_out, uint64_t *blob_off_out, uint8_t *skip_evm_out,
                               uint8_t *data_out);
/* Device-resident form, 1 <= max_blobs <= GSV_MAX_TXS_PER_SHARD.  d_nblobs[i] = the true blob count of
 * body i, also when it exceeds max_blobs; rows [n][max_blobs] of d_blob_start / d_blob_len (uint32) and
 * d_skip_evm (bytes): blob t < min(nblobs, max_blobs) of body i lies at d_data[data_off[i] + blob_start ..
 * + blob_len), later rows are zero.  d_data (may be NULL: index only; 16-byte aligned) holds, per body,
 * every chunk's 31 data bytes at 31 c of the body's data region (so blob_start = 31 first_chunk and no
 * second pass is needed); FILLER BYTES ARE COPIED AS THEY STAND in the body, between one blob's end and
 * the next blob's start.  gsv_blob_data_layout (host arithmetic alone) gives data_off[n + 1]: regions of
 * 31 floor(len / 32) bytes padded to 16, the padding written as zeros. */
int gsv_blob_data_layout(const uint64_t *off, size_t n, uint64_t *data_off_out);
int gsv_blob_deserialize_prepare(gsv_ctx *ctx, const uint64_t *h_off, size_t n, uint32_t max_blobs);
int gsv_blob_deserialize_batch_dev(gsv_ctx *ctx, const uint8_t *d_bodies, const uint64_t *h_off, size_t n,
                                   uint32_t max_blobs, uint32_t *d_nblobs, uint32_t *d_blob_start,
                                   uint32_t *d_blob_len, uint8_t *d_skip_evm, uint8_t *d_data, void *stream);

/* ---- proposer.createCollation (sharding/proposer/proposer.go:55-92) ----
 * Collation i: its encoded transactions are blobs [list_off[i], list_off[i+1]) as above (skip_evm false,
 * convertTxToRawBlob), its header fields shard_id32[i] / period32[i] (32-byte big-endian) and
 * proposer20[i], and the signer's secret key seckey32[i] (the reference takes account and signer
 * separately, and so does this call: the address is not derived from the key).  Per collation:
 *   body           SerializeTxToBlob(txs), at body_off_out[i]: gsv_blob_serialized_size's layout with every
 *                  oversized collation's length 0 (gsv_proposer_body_layout: host arithmetic alone)
 *   chunk_root32   CalculateChunkRoot(); emptyRoot for an empty transaction list
 *   hash32         CollationHeader.Hash() with ProposerSignature empty: what proposer.go:83 signs
 *   sig65          crypto.Sign(hash32, key) = [R || S || V], as gsv_ecdsa_sign_batch returns it
 *   status         GSV_ST_OK; GSV_ST_INVALID_KEY (key 0 or >= n: sig65 zero, body, root and hash still
 *                  produced); GSV_ST_BODY_TOO_LARGE (serialized size > 2^20, collation.go:169-171: a
 *                  zero-length body and zero root, hash and signature; the rest of the batch proceeds)
 * At most 65,535 collations per call.  Steps on the GPU: the serialize kernel, the chunk roots of the
 * bodies it wrote, the header-hash kernel reading those roots, the signing kernel.
 * Secret keys: as for gsv_ecdsa_sign_batch.  The host form stages the keys FIRST in the context's device
 * arena (offset 0) and overwrites that copy, on the context stream and before its final synchronisation,
 * on every return that follows the copy-in (error returns included); it keeps no host copy.  The _dev form
 * reads the caller's device buffer and writes no key material anywhere; wiping that buffer is the caller's.
 * What this path does NOT promise (compare crypto/signature_cgo.go:48-51 on its own caveat): the
 * fixed-base multiplication indexes a 1 GB table in HBM by 20-bit digits of the secret nonce, and the
 * low-s step branches on a bit derived from secrets; libsecp256k1's ecmult_gen is blinded and scans its
 * whole table.  So the path is NOT hardened against a co-tenant that observes timing or memory traffic
 * on the same GPU.  The nonce's inversion mod n is the constant-time one.  Nor does the library control
 * what the HIP runtime's own host-to-device staging buffer holds after a copy from pageable memory. */
int gsv_proposer_body_layout(const uint64_t *blob_off, const uint64_t *list_off, size_t n, uint64_t *body_off_out,
                             uint8_t *status_out);
int gsv_proposer_create_collations(gsv_ctx *ctx, const uint8_t *blobs, const uint64_t *blob_off,
                                   const uint64_t *list_off, size_t n, const uint8_t *shard_id32,
                                   const uint8_t *period32, const uint8_t *proposer20, const uint8_t *seckey32,
                                   uint8_t *bodies_out, uint64_t *body_off_out, uint8_t *chunk_root32_out,
                                   uint8_t *hash32_out, uint8_t *sig65_out, uint8_t *status);
/* Device-resident form: every array in HBM except the two offset tables; d_bodies_out 16-byte aligned.
 * Only enqueues on `stream`; gsv_proposer_prepare prepares it for exactly (blob_off, list_off): the
 * serialize tables, the trie plans of the bodies' lengths and the workspace.  Prepared at pipeline depth
 * D, D calls on D streams run concurrently. */
int gsv_proposer_prepare(gsv_ctx *ctx, const uint64_t *blob_off, const uint64_t *list_off, size_t n);
int gsv_proposer_create_collations_dev(gsv_ctx *ctx, const uint8_t *d_blobs, const uint64_t *blob_off,
                                       const uint64_t *list_off, size_t n, const uint8_t *d_shard_id32,
                                       const uint8_t *d_period32, const uint8_t *d_proposer20,
                                       const uint8_t *d_seckey32, uint8_t *d_bodies_out, uint8_t *d_chunk_root32,
                                       uint8_t *d_hash32, uint8_t *d_sig65, uint8_t *d_status, void *stream);

/* ---- multi-GPU: the shard partition and its one collective ----
 * One process per GPU.  Rank r of N owns the contiguous shard block [floor(S r / N), floor(S (r+1) / N))
 * of S shards (the reference runs one shard per node, --shardid, sharding/node/backend.go:245-284;
 * S = 100 in the SMC, sharding/contracts/sharding_manager.sol:56).
 * gsv_comm_unique_id: rank 0 creates the id and hands it to the other ranks (any channel);
 * gsv_comm_init binds an RCCL communicator (xGMI within the node) to the context's device. */
#define GSV_COMM_ID_BYTES 128
int gsv_comm_unique_id(uint8_t id[GSV_COMM_ID_BYTES]);
int gsv_comm_init(gsv_ctx *ctx, const uint8_t id[GSV_COMM_ID_BYTES], int nranks, int rank);
int gsv_comm_info(gsv_ctx *ctx, int *nranks, int *rank);
/* first shard and shard count of `rank`'s block */
int gsv_shard_range(size_t n_shards, int nranks, int rank, size_t *first, size_t *count);
/* Validates this rank's block (bodies/off: its `count` shards, as gsv_notary_validate_shards) and
 * all-gathers the fixed-size per-shard records over RCCL, so every rank returns the records of all
 * n_total_shards shards in shard order: root32_all[32 S], ntx_all[S], valid_bitmap_all[S ceil(max_txs/8)].
 * senders_out / status_out (optional) cover this rank's own shards only ([count][max_txs]).
 * Needs gsv_comm_init (a context without one behaves as N = 1).
 * Collective contract (as for RCCL itself): every rank calls it with the same n_total_shards, chain id,
 * signer and max_txs.  An error in those returns on every rank before the collective.  A failure local
 * to one rank (its bodies, a body > 2^20 bytes, device memory, a HIP error) does NOT skip the
 * collective: the rank all-gathers an empty block carrying its status, and EVERY rank returns the
 * status of the lowest failing rank (the records of the failing ranks' shards are zero). */
int gsv_notary_validate_partition(gsv_ctx *ctx, const uint8_t *bodies, const uint64_t *off, size_t n_total_shards,
                                  const uint8_t *chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs,
                                  uint8_t *root32_all, uint32_t *ntx_all, uint8_t *valid_bitmap_all,
                                  uint8_t *senders_out, uint8_t *status_out);
/* Device-resident form (the one bench.py times at N > 1): d_bodies holds this rank's block in HBM at the
 * host offsets h_off (count + 1 entries, count from gsv_shard_range); outputs in HBM; enqueues the block's
 * validation, the record pack, one ncclAllGather and the unpack on `stream` and returns.
 * d_rank_status (optional, int32 [nranks]) receives every rank's local status (nonzero: that rank's
 * shards have zero records).  A rank-local failure joins the collective as above and returns its code
 * (the other ranks see it in d_rank_status).  gsv_notary_partition_prepare prepares it for exactly
 * (h_off, n_total_shards, nranks, rank, chain id, signer, max_txs); the context's communicator gives
 * nranks / rank.  Prepared at pipeline depth D (gsv_ctx_set_pipeline_depth), D consecutive calls may be
 * in flight on D streams: their validations overlap, and the library makes each call's all-gather wait
 * for the previous one on the communicator (an event chain; outside a graph capture), so collectives
 * never overlap and every rank issues them in call order. */
int gsv_notary_partition_prepare(gsv_ctx *ctx, const uint64_t *h_off, size_t n_total_shards, int nranks, int rank,
                                 const uint8_t *chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs);
int gsv_notary_validate_partition_dev(gsv_ctx *ctx, const uint8_t *d_bodies, const uint64_t *h_off,
                                      size_t n_total_shards, const uint8_t *chain_id, size_t chain_id_len,
                                      int signer_kind, uint32_t max_txs, uint8_t *d_root32_all, uint32_t *d_ntx_all,
                                      uint8_t *d_valid_bitmap_all, uint8_t *d_senders, uint8_t *d_status,
                                      int32_t *d_rank_status, void *stream);
/* The same two halves for a caller with its own transport (e.g. records gathered across nodes, one
 * shard per node as the reference runs): pack validates rank `rank`'s block and writes its record block
 * (gsv_partition_block_bytes: header {int32 status, uint32 shards} + ceil(S/N) records of
 * root 32 | ntx 4 | bitmap, padded to 8) into d_block; unpack takes the nranks blocks in rank order and
 * writes the per-shard outputs in shard order (+ d_rank_status).  pack needs
 * gsv_notary_partition_prepare with the same (nranks, rank). */
size_t gsv_partition_block_bytes(size_t n_total_shards, int nranks, uint32_t max_txs);
int gsv_notary_partition_pack_dev(gsv_ctx *ctx, const uint8_t *d_bodies, const uint64_t *h_off, size_t n_total_shards,
                                  int nranks, int rank, const uint8_t *chain_id, size_t chain_id_len, int signer_kind,
                                  uint32_t max_txs, uint8_t *d_block, uint8_t *d_senders, uint8_t *d_status,
                                  void *stream);
int gsv_notary_partition_unpack_dev(gsv_ctx *ctx, const uint8_t *d_blocks, size_t n_total_shards, int nranks,
                                    uint32_t max_txs, uint8_t *d_root32_all, uint32_t *d_ntx_all,
                                    uint8_t *d_valid_bitmap_all, int32_t *d_rank_status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSV_H */

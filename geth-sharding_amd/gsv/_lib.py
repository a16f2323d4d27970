"""ctypes binding of libgsv.so (the C ABI in include/gsv.h).

The product path is the HIP library only: if libgsv.so is missing or fails to load this module
raises immediately — there is no CPU fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
# GSV_LIB_PATH overrides the in-tree library (A/B timing of kernel variants only)
LIB_PATH = os.environ.get("GSV_LIB_PATH") or os.path.join(HERE, "libgsv.so")

# status codes (include/gsv.h)
ST_OK = 0
ST_INVALID_MSG_LEN = 1
ST_INVALID_SIG_LEN = 2
ST_INVALID_RECID = 3
ST_RECOVER_FAILED = 4
ST_INVALID_SIG = 5
ST_INVALID_CHAIN_ID = 6
ST_INVALID_PUBKEY = 7
ST_BAD_RLP = 8
ST_BN_BAD_INPUT = 9
ST_PROPOSER_MISMATCH = 10
ST_INVALID_KEY = 11
ST_INVALID_CURVE = 12
ST_BODY_TOO_LARGE = 13
ST_INVALID_MESSAGE = 14
ST_MODEXP_TOO_LONG = 15
ST_INVALID_DIFFICULTY = 16
ST_INVALID_MIX_DIGEST = 17
ST_INVALID_POW = 18
ST_NONCE_NOT_FOUND = 19
ST_HEADER_TOO_WIDE = 20
ST_UNKNOWN_ANCESTOR = 21
ST_EXTRA_TOO_LONG = 22
ST_FUTURE_BLOCK = 23
ST_ZERO_BLOCK_TIME = 24
ST_WRONG_DIFFICULTY = 25
ST_GAS_LIMIT_CAP = 26
ST_GAS_USED = 27
ST_GAS_LIMIT_BOUNDS = 28
ST_INVALID_NUMBER = 29
ST_BAD_PRO_DAO_EXTRA = 30
ST_BAD_NO_DAO_EXTRA = 31
ST_FORK_HASH = 32
ST_RECEIPT_STATUS = 33
ST_GAS_USED_MISMATCH = 34
ST_INVALID_BLOOM = 35
ST_INVALID_RECEIPT_ROOT = 36
ST_BITSET_MISSING_DATA = 37
ST_BITSET_UNREFERENCED_DATA = 38
ST_BITSET_EXCEEDED_TARGET = 39
ST_BITSET_ZERO_CONTENT = 40
ST_CLIQUE_CHECKPOINT_BENEFICIARY = 41
ST_CLIQUE_INVALID_VOTE = 42
ST_CLIQUE_CHECKPOINT_VOTE = 43
ST_CLIQUE_MISSING_VANITY = 44
ST_CLIQUE_MISSING_SIGNATURE = 45
ST_CLIQUE_EXTRA_SIGNERS = 46
ST_CLIQUE_CHECKPOINT_SIGNERS = 47
ST_CLIQUE_MIX_DIGEST = 48
ST_CLIQUE_UNCLE_HASH = 49
ST_CLIQUE_DIFFICULTY = 50
ST_CLIQUE_INVALID_TIMESTAMP = 51
ST_CLIQUE_UNAUTHORIZED = 52
ST_CLIQUE_VOTING_CHAIN = 53

# a short text per per-item status: the reference's error string where it has one (include/gsv.h names
# the sources)
STATUS_STRINGS = {
    ST_OK: "ok",
    ST_INVALID_MSG_LEN: "invalid message length, need 32 bytes",
    ST_INVALID_SIG_LEN: "invalid signature length",
    ST_INVALID_RECID: "invalid signature recovery id",
    ST_RECOVER_FAILED: "recovery failed",
    ST_INVALID_SIG: "invalid transaction v, r, s values",
    ST_INVALID_CHAIN_ID: "invalid chain id for signer",
    ST_INVALID_PUBKEY: "invalid public key",
    ST_BAD_RLP: "rlp: transaction does not decode",
    ST_BN_BAD_INPUT: "bn256: malformed point",
    ST_PROPOSER_MISMATCH: "recovered signer is not the header's proposer",
    ST_INVALID_KEY: "invalid private key",
    ST_INVALID_CURVE: "ecies: invalid elliptic curve",
    ST_BODY_TOO_LARGE: "serialized body size exceeds the collation size limit",
    ST_INVALID_MESSAGE: "ecies: invalid message",
    ST_MODEXP_TOO_LONG: "modexp: a length above GSV_MODEXP_MAX_LEN",
    ST_INVALID_DIFFICULTY: "non-positive difficulty",
    ST_INVALID_MIX_DIGEST: "invalid mix digest",
    ST_INVALID_POW: "invalid proof-of-work",
    ST_NONCE_NOT_FOUND: "ethash: no nonce found within max_attempts",
    ST_HEADER_TOO_WIDE: "header: Difficulty or Time above 32 bytes, or Number above 8",
    ST_UNKNOWN_ANCESTOR: "unknown ancestor",
    ST_EXTRA_TOO_LONG: "extra-data too long",
    ST_FUTURE_BLOCK: "block in the future",
    ST_ZERO_BLOCK_TIME: "timestamp equals parent's",
    ST_WRONG_DIFFICULTY: "invalid difficulty",
    ST_GAS_LIMIT_CAP: "invalid gasLimit",
    ST_GAS_USED: "invalid gasUsed",
    ST_GAS_LIMIT_BOUNDS: "invalid gas limit",
    ST_INVALID_NUMBER: "invalid block number",
    ST_BAD_PRO_DAO_EXTRA: "bad DAO pro-fork extra-data",
    ST_BAD_NO_DAO_EXTRA: "bad DAO no-fork extra-data",
    ST_FORK_HASH: "homestead gas reprice fork: wrong hash",
    ST_RECEIPT_STATUS: "invalid receipt status",
    ST_GAS_USED_MISMATCH: "invalid gas used",
    ST_INVALID_BLOOM: "invalid bloom",
    ST_INVALID_RECEIPT_ROOT: "invalid receipt root hash",
    ST_BITSET_MISSING_DATA: "missing bytes on input",
    ST_BITSET_UNREFERENCED_DATA: "extra bytes on input",
    ST_BITSET_EXCEEDED_TARGET: "target data size exceeded",
    ST_BITSET_ZERO_CONTENT: "zero byte in input content",
    ST_CLIQUE_CHECKPOINT_BENEFICIARY: "beneficiary in checkpoint block non-zero",
    ST_CLIQUE_INVALID_VOTE: "vote nonce not 0x00..0 or 0xff..f",
    ST_CLIQUE_CHECKPOINT_VOTE: "vote nonce in checkpoint block non-zero",
    ST_CLIQUE_MISSING_VANITY: "extra-data 32 byte vanity prefix missing",
    ST_CLIQUE_MISSING_SIGNATURE: "extra-data 65 byte suffix signature missing",
    ST_CLIQUE_EXTRA_SIGNERS: "non-checkpoint block contains extra signer list",
    ST_CLIQUE_CHECKPOINT_SIGNERS: "invalid signer list on checkpoint block",
    ST_CLIQUE_MIX_DIGEST: "non-zero mix digest",
    ST_CLIQUE_UNCLE_HASH: "non empty uncle hash",
    ST_CLIQUE_DIFFICULTY: "invalid difficulty",
    ST_CLIQUE_INVALID_TIMESTAMP: "invalid timestamp",
    ST_CLIQUE_UNAUTHORIZED: "unauthorized",
    ST_CLIQUE_VOTING_CHAIN: "invalid voting chain",
}

SIGNER_EIP155 = 0
SIGNER_HOMESTEAD = 1
SIGNER_FRONTIER = 2

PAIRING_FALSE = 0
PAIRING_TRUE = 1
PAIRING_BAD_INPUT = 2

K_KECCAK = 0
K_ECRECOVER = 1
K_CHUNK_LEAF = 2
K_CHUNK_LEVEL = 3
K_PAIRING = 4
K_SENDER_PREP = 5
K_BN_PREPARE = 6
K_BN_FINAL = 7
K_NOTARY = 8
K_DERIVE_LEAF = 9
K_HEADER = 10
K_BN_G1 = 11
K_ECIES = 12
K_TX_SIGHASH = 13
K_TX_SEAL = 14
K_MODEXP = 15
K_SHA256 = 16
K_RIPEMD160 = 17
K_ETHASH_ITEMS = 18
K_ETHASH_LIGHT = 19
K_TOP = 20  # GSV_K_TOP: pinned; the ids behind it follow
K_ETHASH_FULL = 20
K_ETHASH_SEARCH = 21
K_ETHASH_FINISH = 22
K_PEAK = 23  # GSV_K_PEAK: pinned; the ids behind it follow
K_BLOCK_HEADER = 23
K_BLOCK_RULES = 24
K_BLOCK_MERGE = 25
K_SUMMIT = 26  # GSV_K_SUMMIT: pinned; the ids behind it follow
K_RECEIPT_SCAN = 26
K_RECEIPT_BLOOM = 27
K_RECEIPT_LISTS = 28
K_RECEIPT_CHECK = 29
K_BLOOM9 = 30
K_CREST = 31  # GSV_K_CREST: pinned; the ids behind it follow
K_BLOOMBITS_GENERATE = 31
K_BITSET_COMPRESS = 32
K_BITSET_DECOMPRESS = 33
K_BLOOMBITS_MATCH = 34
K_BLOOMBITS_TOTALS = 35
K_BLOOMBITS_SCAN = 36
K_BLOOMBITS_BLOCKS = 37
K_BLOOM_FILTER = 38
K_RIDGE = 39  # GSV_K_RIDGE: gsv_ctx_kernel_time takes every id below it

CLIQUE_RECORD_BYTES = 128  # the record of one header gsv_clique_fold reads (include/gsv.h "clique")

ETHASH_MAX_CACHES = 3  # GSV_ETHASH_MAX_CACHES: epoch caches a context keeps for the ethash host forms
ETHASH_MAX_DATASETS = 2  # GSV_ETHASH_MAX_DATASETS: epoch datasets a context keeps for the full and seal forms

BLOOMBITS_MAX_SECTION = 32768  # GSV_BLOOMBITS_MAX_SECTION: blooms of one section, a multiple of 8 from 8 up
BLOOM_BITS = 2048  # GSV_BLOOM_BITS: bit vectors of a section
BITSET_MAX_LEN = 4096  # GSV_BITSET_MAX_LEN: the longest vector the bitset codec takes

MODEXP_MAX_LEN = 1024  # GSV_MODEXP_MAX_LEN: the cap on baseLen, expLen and modLen of the modexp precompile


def tx_sign_growth(chain_id_len: int) -> int:
    """GSV_TX_SIGN_GROWTH: the signed encoding of a transaction is at most this much longer than its input"""
    return int(chain_id_len) + 67

ECIES_OVERHEAD = 113  # GSV_ECIES_OVERHEAD: 65 (R) + 16 (IV) + 32 (tag)

# API errors (negative return values)
E_INVALID_ARG = -1
E_HIP = -2
E_NOMEM = -3
E_NO_DEVICE = -4
E_TOO_LARGE = -5
E_RCCL = -6
E_NOT_PREPARED = -7

MAX_STREAMS = 8  # GSV_MAX_STREAMS: live gsv_stream_create streams per context

_u8p = ctypes.POINTER(ctypes.c_uint8)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_u64 = ctypes.c_uint64


class ChainConfigStruct(ctypes.Structure):
    """gsv_chain_config (include/gsv.h): the fields of params.ChainConfig the header rules read"""
    _fields_ = [("homestead_block", ctypes.c_uint64), ("dao_fork_block", ctypes.c_uint64),
                ("eip150_block", ctypes.c_uint64), ("byzantium_block", ctypes.c_uint64),
                ("has_homestead", ctypes.c_uint8), ("has_dao_fork", ctypes.c_uint8), ("has_eip150", ctypes.c_uint8),
                ("has_byzantium", ctypes.c_uint8), ("dao_fork_support", ctypes.c_uint8),
                ("reserved", ctypes.c_uint8 * 3), ("eip150_hash", ctypes.c_uint8 * 32)]


class CliqueConfigStruct(ctypes.Structure):
    """gsv_clique_config (include/gsv.h): params.CliqueConfig"""
    _fields_ = [("period", ctypes.c_uint64), ("epoch", ctypes.c_uint64)]


# (name, restype, argtypes) for every symbol declared in include/gsv.h
SIGNATURES = [
    ("gsv_device_count", ctypes.c_int, []),
    ("gsv_ctx_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    ("gsv_ctx_destroy", None, [_vp]),
    ("gsv_error_string", ctypes.c_char_p, [ctypes.c_int]),
    ("gsv_abi_version", ctypes.c_int, []),
    ("gsv_ctx_set_timing", ctypes.c_int, [_vp, ctypes.c_int]),
    ("gsv_ctx_kernel_time", ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_long)]),
    ("gsv_ctx_reset_timing", ctypes.c_int, [_vp]),
    ("gsv_keccak256_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("gsv_keccak256_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_sha256_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("gsv_sha256_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ripemd160_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("gsv_ripemd160_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ecrecover_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ecrecover_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("gsv_ecdsa_verify_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    ("gsv_ecdsa_verify_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_pubkey_parse_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_pubkey_parse_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ecdsa_sign_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ecdsa_sign_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_pubkey_create_batch", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_pubkey_create_batch_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("gsv_secp256k1_scalar_mul_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_secp256k1_scalar_mul_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ecdh_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ecdh_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("gsv_ctx_arena_read", ctypes.c_int, [_vp, _sz, _sz, _vp]),
    ("gsv_ecies_decrypt_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ecies_encrypt_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ecies_work_bytes", _sz, [_sz, ctypes.c_int]),
    ("gsv_ecies_decrypt_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_ecies_encrypt_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("gsv_sender_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_int, _vp, _vp]),
    ("gsv_tx_sender_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int, _vp, _vp]),
    ("gsv_tx_sign_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("gsv_tx_sign_work_bytes", _sz, [_sz]),
    ("gsv_tx_sign_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _sz, ctypes.c_int, _vp, _vp, _vp, _vp,
                                             _vp, _vp]),
    ("gsv_chunk_root_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("gsv_chunk_root_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_bn256_pairing_check_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("gsv_bn256_pairing_check_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_bn256_synth_checks_dev", ctypes.c_int, [_vp, ctypes.c_uint64, _sz, _vp, _vp, _vp]),
    ("gsv_synth_sign", ctypes.c_int, [_vp, ctypes.c_uint64, _sz, _vp, _vp, _vp, _vp]),
    ("gsv_synth_sign_dev", ctypes.c_int, [_vp, ctypes.c_uint64, _sz, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_notary_validate_shards", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int, ctypes.c_uint32,
                                                  _vp, _vp, _vp, _vp, _vp]),
    ("gsv_notary_validate_shards_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int,
                                                      ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_notary_synth_dev", ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32, _sz, ctypes.c_uint32, _vp, _vp,
                                            _vp, _vp]),
    ("gsv_derive_sha_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp]),
    ("gsv_derive_sha_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_collation_poc_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    ("gsv_collation_poc_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    ("gsv_collation_header_verify_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_collation_header_verify_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp,
                                                             _vp]),
    ("gsv_ctx_prepared_shapes", ctypes.c_int, [_vp, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    ("gsv_ctx_set_pipeline_depth", ctypes.c_int, [_vp, ctypes.c_int]),
    ("gsv_stream_create", ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    ("gsv_stream_destroy", ctypes.c_int, [_vp, _vp]),
    ("gsv_ctx_stream_count", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("gsv_ecrecover_precompile_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ecrecover_precompile_batch_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_bn256_add_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_bn256_add_batch_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_bn256_scalar_mul_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_bn256_scalar_mul_batch_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_modexp_output_layout", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp]),
    ("gsv_modexp_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_modexp_work_bytes", _sz, [_sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    ("gsv_modexp_batch_dev", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp,
                                            _vp]),
    ("gsv_ethash_cache_size", _u64, [_u64]),
    ("gsv_ethash_dataset_size", _u64, [_u64]),
    ("gsv_ethash_seed_hash", ctypes.c_int, [_u64, _vp]),
    ("gsv_ethash_make_cache", ctypes.c_int, [_vp, _u64, _vp]),
    ("gsv_ethash_dataset_items_dev", ctypes.c_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp]),
    ("gsv_ethash_light_batch_dev", ctypes.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ethash_verify_seal_batch_dev", ctypes.c_int, [_vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ethash_light_batch", ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ethash_verify_seal_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, ctypes.c_int, _vp]),
    ("gsv_ctx_ethash_caches", ctypes.c_int, [_vp, ctypes.POINTER(_sz)]),
    ("gsv_ethash_full_batch_dev", ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_ethash_verify_seal_full_batch_dev", ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ethash_search_dev", ctypes.c_int, [_vp, _vp, _u64, _vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_ethash_full_batch", ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ethash_seal_batch", ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, _vp, _sz, _u64, _vp, _vp, _vp]),
    ("gsv_ctx_ethash_datasets", ctypes.c_int, [_vp, ctypes.POINTER(_sz)]),
    ("gsv_block_header_hash_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    ("gsv_calc_difficulty_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_ethash_verify_headers_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _u64, ctypes.c_int, _vp,
                                                       _vp, _vp]),
    ("gsv_block_header_work_bytes", _sz, [_sz]),
    ("gsv_block_header_rules_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _sz, _u64, _vp, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp]),
    ("gsv_block_header_merge_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_clique_snapshot_new", _vp, [_vp, _sz, _u64, _vp]),
    ("gsv_clique_snapshot_from_genesis", _vp, [_vp, _sz, ctypes.POINTER(ctypes.c_int)]),
    ("gsv_clique_snapshot_copy", _vp, [_vp]),
    ("gsv_clique_snapshot_free", None, [_vp]),
    ("gsv_clique_snapshot_number", _u64, [_vp]),
    ("gsv_clique_snapshot_hash", ctypes.c_int, [_vp, _vp]),
    ("gsv_clique_snapshot_signers", _sz, [_vp, _vp, _sz]),
    ("gsv_clique_snapshot_recents", _sz, [_vp, _vp, _vp, _sz]),
    ("gsv_clique_snapshot_votes", _sz, [_vp, _vp, _vp, _vp, _vp, _sz]),
    ("gsv_clique_snapshot_tally", _sz, [_vp, _vp, _vp, _vp, _sz]),
    ("gsv_clique_snapshot_inturn", ctypes.c_int, [_vp, _u64, _vp]),
    ("gsv_clique_calc_difficulty", ctypes.c_int, [_vp, _vp]),
    ("gsv_clique_fold", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, ctypes.POINTER(_sz)]),
    ("gsv_bloom9_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    ("gsv_bloom9_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_receipts_work_bytes", _sz, [_sz, _u64]),
    ("gsv_receipts_bloom_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_receipts_check_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_receipts_verify_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_bloombits_generate_batch", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_uint32, _vp]),
    ("gsv_bloombits_generate_dev", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_uint32, _vp, _vp]),
    ("gsv_bitset_compress_batch", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_uint32, _vp, _vp]),
    ("gsv_bitset_compress_batch_dev", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp]),
    ("gsv_bitset_decompress_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp]),
    ("gsv_bitset_decompress_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp]),
    ("gsv_bloombits_match_dev", ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _u64, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp,
                                               _vp, _vp, _vp, _vp]),
    ("gsv_bloombits_blocks_dev", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _u64, _sz, _sz, _vp, _vp, _u64, _vp]),
    ("gsv_bloombits_match_batch", ctypes.c_int, [_vp, _vp, ctypes.c_uint32, _u64, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp,
                                                 _vp, _vp, _vp, _u64]),
    ("gsv_bloom_filter_dev", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp]),
    ("gsv_bloom_filter_batch", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    ("gsv_chunk_root_prepare", ctypes.c_int, [_vp, _vp, _sz]),
    ("gsv_bn256_pairing_prepare", ctypes.c_int, [_vp, _vp, _sz]),
    ("gsv_notary_prepare", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz, ctypes.c_int, ctypes.c_uint32]),
    ("gsv_derive_sha_prepare", ctypes.c_int, [_vp, _vp, _vp, _sz]),
    ("gsv_collation_poc_prepare", ctypes.c_int, [_vp, _vp, _sz, _vp, _sz]),
    ("gsv_collation_header_prepare", ctypes.c_int, [_vp, _sz]),
    ("gsv_comm_unique_id", ctypes.c_int, [_vp]),
    ("gsv_comm_init", ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int]),
    ("gsv_comm_info", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("gsv_shard_range", ctypes.c_int, [_sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    ("gsv_notary_validate_partition", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int, ctypes.c_uint32,
                                                     _vp, _vp, _vp, _vp, _vp]),
    ("gsv_notary_partition_prepare", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _vp, _sz,
                                                    ctypes.c_int, ctypes.c_uint32]),
    ("gsv_notary_validate_partition_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _sz, ctypes.c_int, ctypes.c_uint32,
                                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("gsv_partition_block_bytes", _sz, [_sz, ctypes.c_int, ctypes.c_uint32]),
    ("gsv_notary_partition_pack_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_int, ctypes.c_int, _vp, _sz,
                                                     ctypes.c_int, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    ("gsv_notary_partition_unpack_dev", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, ctypes.c_uint32, _vp, _vp, _vp,
                                                       _vp, _vp]),
    ("gsv_blob_serialized_size", ctypes.c_int, [_vp, _vp, _sz, _vp]),
    ("gsv_blob_serialize_batch", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_blob_serialize_prepare", ctypes.c_int, [_vp, _vp, _vp, _sz]),
    ("gsv_blob_serialize_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    ("gsv_blob_deserialize_batch", ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    ("gsv_blob_data_layout", ctypes.c_int, [_vp, _sz, _vp]),
    ("gsv_blob_deserialize_prepare", ctypes.c_int, [_vp, _vp, _sz, ctypes.c_uint32]),
    ("gsv_blob_deserialize_batch_dev", ctypes.c_int, [_vp, _vp, _vp, _sz, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                                      _vp]),
    ("gsv_proposer_body_layout", ctypes.c_int, [_vp, _vp, _sz, _vp, _vp]),
    ("gsv_proposer_create_collations", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                      _vp, _vp, _vp]),
    ("gsv_proposer_prepare", ctypes.c_int, [_vp, _vp, _vp, _sz]),
    ("gsv_proposer_create_collations_dev", ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                          _vp, _vp, _vp]),
]

_lib = None
_lock = threading.Lock()


class GsvError(RuntimeError):
    """A negative GSV_E_* return value from the library (`code`)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load():
    """Load libgsv.so (raises OSError loudly if it is not built)."""
    global _lib
    with _lock:
        if _lib is None:
            # PyTorch-ROCm ships its own libamdhip64; when both runtimes live in one process,
            # torch's must initialise first or torch later finds no GPU.  Importing torch here (when
            # installed) makes the order independent of what the caller imported first.
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
            if not os.path.exists(LIB_PATH):
                raise OSError(f"libgsv.so not built at {LIB_PATH}: run `make -C geth-sharding_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback")
            L = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                f = getattr(L, name, None)
                if f is None:  # reported by tests/test_abi.py; calling it raises AttributeError
                    continue
                f.restype = res
                f.argtypes = args
            _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        msg = load().gsv_error_string(rc).decode()
        raise GsvError(f"libgsv error {rc}: {msg}", rc)

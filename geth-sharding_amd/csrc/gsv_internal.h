// Internal declarations shared by the HIP translation units of libgsv.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsv.h"
#include "block_header_host.h"

namespace gsv {

// ecrecover.hip
hipError_t launch_gtable_init(uint4* gtab, hipStream_t st);
hipError_t launch_ecrecover(const uint8_t* msg32, const uint8_t* sig65, uint32_t n, const uint4* gtab,
                            uint8_t* pub65, uint8_t* addr20, uint8_t* status, hipStream_t st);
hipError_t launch_sender(const uint8_t* sighash32, const uint8_t* r32, const uint8_t* s32,
                         const uint64_t* v, const uint8_t* vbig, uint32_t n, int homestead,
                         const uint4* gtab, uint8_t* addr20, uint8_t* status, hipStream_t st);
hipError_t launch_ecrecover_precompile(const uint8_t* in128, uint32_t n, const uint4* gtab, uint8_t* out32,
                                       uint8_t* ok, hipStream_t st);
hipError_t launch_synth_sign(uint64_t seed, uint32_t n, const uint4* gtab, uint8_t* msg32,
                             uint8_t* sig65, uint8_t* pub65, uint8_t* addr20, hipStream_t st);

// ecverify.hip: keys as n x 65-byte rows plus a length byte each (pubkey_pack.h)
hipError_t launch_ecverify(const uint8_t* msg32, const uint8_t* sig64, const uint8_t* pub65, const uint8_t* publen,
                           uint32_t n, const uint4* gtab, uint8_t* ok, hipStream_t st);
hipError_t launch_pubkey_parse(const uint8_t* pub65, const uint8_t* publen, uint32_t n, uint8_t* out65, uint8_t* ok,
                               hipStream_t st);

// ecsign.hip: crypto.Sign (RFC 6979 nonce) and secp256k1_ec_pubkey_create; status GSV_ST_OK / GSV_ST_INVALID_KEY
hipError_t launch_ecsign(const uint8_t* msg32, const uint8_t* seckey32, uint32_t n, const uint4* gtab, uint8_t* sig65,
                         uint8_t* status, hipStream_t st);
hipError_t launch_pubkey_create(const uint8_t* seckey32, uint32_t n, const uint4* gtab, uint8_t* pub65,
                                uint8_t* addr20, uint8_t* status, hipStream_t st);

// txsign.hip: the two kernels of types.SignTx around launch_ecsign.  What they need of the signer and the
// chain id is prepared on the host (gsv_txsign.hip) and passed by value:
//   TxSignSuffix  what the signer's Hash appends to the six fields: rlp(chainId) 80 80 for EIP-155 (at
//                 most 68 bytes), nothing for Homestead / Frontier.  Word 0 is zero, byte j of the suffix
//                 is byte 4 + j of w, zero behind it (tx_flat.cuh TxStream's tail layout).
//   TxSignVTable  the RLP item of V for recovery id 0..3 (row r: TXS_V_WORDS zero-padded words, len[r]
//                 bytes, at most 67).
// rec: a uint4 per item {segment offset, segment length, recipient patch offset, status}.
constexpr uint32_t TXS_SUFFIX_WORDS = 20, TXS_V_WORDS = 17;
struct TxSignSuffix {
    uint32_t w[TXS_SUFFIX_WORDS];
    uint32_t len;
};
struct TxSignVTable {
    uint32_t w[4 * TXS_V_WORDS];
    uint32_t len[4];
};
// the caller's work area of the _dev form (gsv_tx_sign_work_bytes), no padding between its parts:
// rec 16 n | msg32 32 n | sig65 65 n | sign status n
constexpr size_t TXS_WORK_PER = 16 + 32 + 65 + 1;
hipError_t launch_tx_sighash(const uint8_t* d_rlp, const uint64_t* d_off, uint32_t n, const TxSignSuffix& sfx,
                             uint32_t* d_rec, uint32_t* d_msg32, hipStream_t st);
hipError_t launch_tx_seal(const uint8_t* d_rlp, const uint64_t* d_off, uint32_t n, const TxSignVTable& vt,
                          uint64_t growth, const uint32_t* d_rec, const uint8_t* d_sig65, const uint8_t* d_sign_st,
                          uint8_t* d_out, uint32_t* d_out_len, uint8_t* d_hash32, uint8_t* d_status, hipStream_t st);

// ecdh.hip: secp256k1_ext_scalar_mul and what ECIES derives from its X.  Outputs that are null are not
// written: xy64 (X || Y), x32 (X), keys48 (Ke || Km); status GSV_ST_OK / GSV_ST_INVALID_KEY /
// GSV_ST_INVALID_CURVE
hipError_t launch_ecdh(const uint8_t* point64, const uint8_t* scalar32, uint32_t n, uint8_t* xy64, uint8_t* x32,
                       uint8_t* keys48, uint8_t* status, hipStream_t st);

// ecies.hip: the launches of Decrypt / Encrypt around launch_ecdh (launch_pubkey_create too for
// Encrypt).  work: the caller's area they share, no padding between its parts (ecies.hip draws it):
// ECIES_WORK_DEC / ECIES_WORK_ENC bytes per item
constexpr size_t ECIES_WORK_DEC = 48 + 64 + 1, ECIES_WORK_ENC = 48 + 65 + 1 + 1;
hipError_t launch_ecies_parse(const uint8_t* ct, const uint64_t* ct_off, const uint8_t* seckey32, uint32_t n,
                              uint8_t* point64, uint8_t* status, hipStream_t st);
hipError_t launch_ecies_open(const uint8_t* ct, const uint64_t* ct_off, const uint8_t* s2, const uint64_t* s2_off,
                             uint32_t n, uint8_t* work, uint8_t* msg_out, uint32_t* msg_len, uint8_t* status,
                             hipStream_t st);
hipError_t launch_ecies_seal(const uint8_t* msg, const uint64_t* msg_off, const uint8_t* iv16, const uint8_t* s2,
                             const uint64_t* s2_off, uint32_t n, uint8_t* work, uint8_t* ct_out, uint8_t* status,
                             hipStream_t st);

// keccak.hip
hipError_t launch_keccak256(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out32,
                            hipStream_t st);

// hash_md.hip: SHA-256 rows, and RIPEMD-160 rows of 12 zero bytes and the 20-byte digest
hipError_t launch_sha256(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out32, hipStream_t st);
hipError_t launch_ripemd160(const uint8_t* data, const uint64_t* off, uint32_t n, uint8_t* out32, hipStream_t st);

// Launchers call timer_begin(tctx, GSV_HOOK_TAIL) (no launch follows it directly) where the call's
// bulk kernels end and its latency-bound tail begins (trie top, Miller loop + final exponentiation):
// with pipelined shape instances the next call's bulk kernels start there (gsv_ctx.h shape_run).
constexpr int GSV_HOOK_TAIL = -1;

// chunk_root.hip
struct TriePlan;  // host-built, device-resident trie shape for one body length N
size_t chunk_root_scratch_bytes(const TriePlan* plan, uint32_t nbodies);
hipError_t launch_chunk_root_plan(const TriePlan* plan, const uint8_t* d_bodies, const uint64_t* d_body_off,
                                  uint32_t nbodies, uint8_t* d_scratch, uint8_t* d_roots, hipStream_t st,
                                  void (*timer_begin)(void*, int), void (*timer_end)(void*, int),
                                  void* tctx);

// generic DeriveSha (any DerivableList) and the Proof-of-Custody salted body
size_t derive_sha_scratch_bytes(const TriePlan* plan, uint32_t nlists);
hipError_t launch_derive_sha_plan(const TriePlan* plan, uint32_t nlists, const uint8_t* d_vals,
                                  const uint64_t* d_voff, uint64_t vend, const uint64_t* d_leaf_base, uint8_t* d_lmsg, uint8_t* d_leafrefs, uint8_t* d_scratch, uint8_t* d_roots,
                                  hipStream_t st, void (*timer_begin)(void*, int), void (*timer_end)(void*, int),
                                  void* tctx);
hipError_t launch_poc_expand(const uint8_t* d_bodies, const uint64_t* d_in_off, const uint64_t* d_out_off,
                             uint32_t nbodies, uint64_t max_out, const uint8_t* d_salt, uint32_t slen, uint8_t* d_out,
                             hipStream_t st);

// collation.hip: header hashes + proposer signature (ecrecover of the unsigned header hash)
size_t header_scratch_bytes(uint32_t n);
hipError_t launch_header_verify(const uint8_t* d_sid32, const uint8_t* d_root32, const uint8_t* d_per32,
                                const uint8_t* d_prop20, const uint8_t* d_sig65, const uint8_t* d_nil, uint32_t n,
                                const uint4* gtab, uint8_t* d_scratch, uint8_t* d_hash32, uint8_t* d_signer20,
                                uint8_t* d_status, hipStream_t st);

// layout flags of launch_bn256_pairing: the final exponentiation on three lanes per check and the Miller
// loop on two lanes per Miller lane (batches below one wave per SIMD), the two-wave lines kernel
// (LINESW2, large batches; else the one-wave k_bn_lines), and the two-wave Miller kernels kept for A/B
// (MILLERW2, MILLERL; off by default)
constexpr int GSV_BN_LAYOUT_FINAL3 = 1, GSV_BN_LAYOUT_MILLER2 = 2, GSV_BN_LAYOUT_MILLERW2 = 8,
              GSV_BN_LAYOUT_LINESW2 = 16, GSV_BN_LAYOUT_MILLERL = 32;
// bn256.hip: pairs in slot-major order (the j-th pairs of all checks contiguous): pair_src[p] = byte
// offset of pair p in d_in.  A check's pairs are split into Miller lanes of <= k pairs each: lane l
// runs the multi-Miller loop over pidx[lane_first[l] .. lane_first[l+1]), check c owns lanes
// [check_lane[c], check_lane[c+1]); cbad[c] != 0 marks a ragged input length (no pairs, verdict
// BAD_INPUT).  Workspaces (F_p elements are 9 words, bn254_fe9.cuh): pstat[npairs],
// lines[91 * 54][npairs], lstat[nlanes], fv[108][nlanes] words, fws[BN_FINAL_SLOTS * 108][nchecks]
// words (the final exponentiation's values that outlive its registers); maxl = the most lanes any
// check has.  final3: the final exponentiation runs on three cooperating lanes per check (small batches)
constexpr int BN_FINAL_SLOTS = 8;
hipError_t launch_bn256_pairing(const uint8_t* d_in, const uint64_t* d_pair_src, uint32_t npairs,
                                const uint32_t* d_lane_first, const uint32_t* d_pidx, uint32_t nlanes,
                                const uint32_t* d_check_lane, const uint8_t* d_cbad, uint32_t nchecks,
                                uint8_t* d_pstat, uint32_t* d_lines, uint8_t* d_lstat, uint32_t* d_fv,
                                uint32_t* d_fws, uint32_t maxl, uint8_t* d_verdict, int layout, hipStream_t st, void (*timer_begin)(void*, int),
                                void (*timer_end)(void*, int), void* tctx);
hipError_t launch_bn256_synth(uint64_t seed, uint32_t nchecks, uint8_t* d_out, uint8_t* d_expect, hipStream_t st);

// bn_g1.hip: the bn256Add / bn256ScalarMul precompiles over fixed-size records (128 B / 96 B -> 64 B +
// status).  bitserial != 0 selects the 256-step double-and-add form of the multiplication (the A/B
// partner of the GLV path: tools/bn_g1_sweep.py and the tests only)
hipError_t launch_bn256_g1_add(const uint8_t* d_in128, uint32_t n, uint8_t* d_out64, uint8_t* d_status,
                               hipStream_t st);
hipError_t launch_bn256_g1_mul(const uint8_t* d_in96, uint32_t n, uint8_t* d_out64, uint8_t* d_status,
                               int bitserial, hipStream_t st);

// modexp.hip: the bigModExp precompile over n rows of base || exp || mod (bl + el + ml bytes, each length
// <= 1024), n rows of ml bytes out; d_work = mdx::work_bytes(n, ml) bytes (modexp_plan.h), 4-byte aligned
hipError_t launch_modexp(const uint8_t* d_in, uint32_t n, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* d_out,
                         uint8_t* d_work, hipStream_t st);

// ethash.hip: dataset items [first, first + count), hashimotoLight and VerifySeal over a device-resident cache
// of cache_bytes (a multiple of 64, 16-byte aligned) and a dataset of dataset_bytes (a multiple of 128, at
// most 2^38); hash rows 4-byte and nonces 8-byte aligned, d_out64 16-byte aligned
hipError_t launch_ethash_items(const uint8_t* d_cache, uint64_t cache_bytes, uint32_t first, uint32_t count,
                               uint8_t* d_out64, hipStream_t st);
hipError_t launch_ethash_light(const uint8_t* d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                               const uint8_t* d_hash32, const uint64_t* d_nonce, uint32_t n, uint8_t* d_mix32,
                               uint8_t* d_result32, hipStream_t st);
hipError_t launch_ethash_verify(const uint8_t* d_cache, uint64_t cache_bytes, uint64_t dataset_bytes,
                                const uint8_t* d_hash32, const uint64_t* d_nonce, const uint8_t* d_mix32,
                                const uint8_t* d_difficulty32, uint32_t n, uint8_t* d_status, hipStream_t st);
// the same over the dataset itself (128-byte aligned, dataset_bytes of it); search: n headers x span nonces
// from d_start[h], n * ceil(span / 256) workgroups, d_offset[h] pre-set to 0xFFFFFFFF; finish: the rows of
// nonce d_start[h] + d_offset[h] where an offset was left, zeros and d_found[h] = 0 elsewhere
hipError_t launch_ethash_full(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                              const uint64_t* d_nonce, uint32_t n, uint8_t* d_mix32, uint8_t* d_result32,
                              hipStream_t st);
hipError_t launch_ethash_verify_full(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                                     const uint64_t* d_nonce, const uint8_t* d_mix32, const uint8_t* d_difficulty32,
                                     uint32_t n, uint8_t* d_status, hipStream_t st);
hipError_t launch_ethash_search(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                                const uint8_t* d_difficulty32, const uint64_t* d_start, uint32_t n, uint32_t span,
                                uint32_t* d_offset, hipStream_t st);
hipError_t launch_ethash_finish(const uint8_t* d_dataset, uint64_t dataset_bytes, const uint8_t* d_hash32,
                                const uint64_t* d_start, const uint32_t* d_offset, uint32_t n, uint64_t* d_nonce_out,
                                uint8_t* d_mix32, uint8_t* d_result32, uint8_t* d_found, hipStream_t st);

// block_header.hip: types.Header decode + Hash / HashNoNonce into the records of d_work (bh::work_bytes(n) bytes, 16-byte
// aligned; entry n is the parent of header 0, parent_len == 0: none), the rules of verifyHeader around the seal, the
// merge of the three statuses, and CalcDifficulty alone over n decoded parents.  Output rows that are null are not
// written; d_hnn32 is 4-byte and d_nonce / d_number / d_time 8-byte aligned
hipError_t launch_block_header(const uint8_t* d_rlp, const uint64_t* d_off, uint32_t n, const uint8_t* d_parent_rlp,
                               uint32_t parent_len, uint8_t* d_work, uint8_t* d_hash32, uint8_t* d_hnn32,
                               uint64_t* d_nonce, uint8_t* d_mix32, uint8_t* d_difficulty32, uint64_t* d_number,
                               uint8_t* d_status, hipStream_t st);
hipError_t launch_block_header_rules(uint8_t* d_work, uint32_t n, const bh::Config& cfg, uint64_t now, uint8_t* d_pre,
                                     uint8_t* d_post, uint8_t* d_want32, hipStream_t st);
hipError_t launch_block_header_merge(const uint8_t* d_pre, const uint8_t* d_seal, const uint8_t* d_seals,
                                     const uint8_t* d_post, uint32_t n, uint8_t* d_status, hipStream_t st);
hipError_t launch_calc_difficulty(uint8_t* d_work, uint32_t n, const bh::Config& cfg, const uint64_t* d_time,
                                  uint8_t* d_want32, uint8_t* d_status, hipStream_t st);

// receipt.hip: the receipt half of ValidateState.  d_work: rc::work_bytes(n, vals_bytes) bytes (receipt_host.h),
// 8-byte aligned, its descriptor table zero-filled before the scan; the bloom rows (256 bytes each, any alignment)
// zero-filled before the bloom launch; d_receipt_bloom null: not wanted
hipError_t launch_receipt_scan(const uint8_t* d_vals, const uint64_t* d_voff, uint32_t n, const uint64_t* d_list_off,
                               uint32_t n_lists, uint64_t vals_bytes, uint8_t* d_work, uint8_t* d_receipt_status,
                               hipStream_t st);
hipError_t launch_receipt_bloom(const uint8_t* d_vals, const uint64_t* d_voff, uint32_t n, uint64_t vals_bytes,
                                const uint8_t* d_work, uint8_t* d_list_bloom, uint8_t* d_receipt_bloom,
                                hipStream_t st);
hipError_t launch_receipt_lists(const uint64_t* d_list_off, uint32_t n_lists, uint32_t n, uint64_t vals_bytes,
                                const uint8_t* d_work, const uint8_t* d_receipt_status, uint8_t* d_list_bloom,
                                uint64_t* d_gas_used, uint8_t* d_list_status, hipStream_t st);
hipError_t launch_receipt_check(const uint8_t* d_list_status, uint32_t n_lists, const uint8_t* d_list_bloom,
                                uint8_t* d_root32, const uint64_t* d_gas_used, const uint8_t* d_want_bloom,
                                const uint8_t* d_want_root32, const uint64_t* d_want_gas, uint8_t* d_status,
                                hipStream_t st);
// bloom9's three bit numbers per message: d_idx n x 3 uint16
hipError_t launch_bloom9(const uint8_t* d_data, const uint64_t* d_off, uint32_t n, uint16_t* d_idx, hipStream_t st);

// bloombits.hip: the section generator, the bitset codec, the matcher and bloomFilter (include/gsv.h "bloombits";
// the bounds are bloombits_host.h's).  Byte arrays have any alignment; offsets and counts their natural one.
hipError_t launch_bloombits_generate(const uint8_t* d_blooms, uint32_t n_sections, uint32_t S, uint8_t* d_bits,
                                     hipStream_t st);
hipError_t launch_bitset_compress(const uint8_t* d_in, uint32_t n, uint32_t L, uint8_t* d_slots, uint32_t* d_len,
                                  hipStream_t st);
hipError_t launch_bitset_decompress(const uint8_t* d_data, const uint64_t* d_off, uint32_t n, uint32_t L, uint8_t* d_out,
                                    uint8_t* d_status, hipStream_t st);
hipError_t launch_bloombits_match(const uint8_t* d_bits, uint32_t S, uint64_t first_section, uint32_t n_sections,
                                  const uint16_t* d_clauses, uint32_t n_clauses, const uint32_t* d_rule_off,
                                  uint32_t n_rules, const uint32_t* d_query_off, uint32_t n_queries,
                                  const uint64_t* d_begin, const uint64_t* d_end, uint8_t* d_match, uint32_t* d_count,
                                  hipStream_t st);
hipError_t launch_bloombits_totals(const uint32_t* d_count, uint32_t n_sections, uint32_t n_queries,
                                   uint64_t* d_block_off, hipStream_t st);
hipError_t launch_bloombits_scan(uint64_t* d_block_off, uint32_t n_queries, hipStream_t st);
hipError_t launch_bloombits_blocks(const uint8_t* d_match, const uint32_t* d_count, uint32_t S, uint64_t first_section,
                                   uint32_t n_sections, uint32_t n_queries, const uint64_t* d_block_off,
                                   uint64_t* d_blocks, uint64_t capacity, hipStream_t st);
hipError_t launch_bloom_filter(const uint8_t* d_blooms, uint32_t n_blooms, const uint16_t* d_clauses, uint32_t n_clauses,
                               const uint32_t* d_rule_off, uint32_t n_rules, const uint32_t* d_query_off,
                               uint32_t n_queries, uint8_t* d_out, hipStream_t st);

// collation.hip: CollationHeader.Hash() with ProposerSignature empty (k_header_hash alone: the hash the
// proposer signs), no nil fields
hipError_t launch_header_hash_unsigned(const uint8_t* d_sid32, const uint8_t* d_root32, const uint8_t* d_per32,
                                       const uint8_t* d_prop20, uint32_t n, uint8_t* d_hash32, hipStream_t st);

// blob.hip: the blob codec (blob_codec.h) and the proposer's mask.  d_ents: blobc::BlobEnt per blob;
// d_chunk_blob: the blob of each output chunk; output and data regions 16-byte aligned
hipError_t launch_blob_serialize(const uint8_t* d_blobs, uint64_t begin, uint64_t end, const void* d_ents,
                                 const uint32_t* d_chunk_blob, const uint8_t* d_skip_evm, uint64_t nchunks,
                                 uint8_t* d_out, hipStream_t st);
hipError_t launch_blob_strip(const uint8_t* d_bodies, uint64_t begin, uint64_t end, const uint64_t* d_body_off,
                             const uint32_t* d_body_len, const uint64_t* d_data_off, uint32_t n, uint64_t max_region,
                             uint8_t* d_data, hipStream_t st);
hipError_t launch_blob_unpack(const void* d_recs, const uint32_t* d_cnt, uint32_t n, uint32_t max_blobs,
                              uint32_t* d_start, uint32_t* d_len, uint8_t* d_skip, hipStream_t st);
hipError_t launch_proposer_mask(const uint8_t* d_over, uint32_t n, uint8_t* d_root32, uint8_t* d_hash32,
                                uint8_t* d_sig65, uint8_t* d_status, hipStream_t st);

// notary.hip
struct BlobRec {  // k_blob_index's record of one blob
    uint32_t first_chunk;  // chunk index in the shard body
    uint32_t nchunks;
    uint32_t len;          // data bytes = 31 * (nchunks - 1) + terminal length
    uint32_t skip_evm;
};
size_t blob_rec_bytes();
hipError_t launch_partition_pack(const uint8_t* d_root, const uint32_t* d_ntx, const uint8_t* d_bm, uint32_t n,
                                 uint32_t per, uint32_t R, uint32_t bm, int32_t status, uint8_t* d_block,
                                 hipStream_t st);
hipError_t launch_partition_unpack(const uint8_t* d_all, uint32_t nranks, uint32_t n_total, uint32_t R, uint32_t bm,
                                   size_t B, uint8_t* d_root, uint32_t* d_ntx, uint8_t* d_bm, int32_t* d_rank_status,
                                   hipStream_t st);
hipError_t launch_blob_index(const uint8_t* d_bodies, const uint64_t* d_off, const uint32_t* d_len,
                             uint32_t n_shards, uint32_t max_txs, void* d_blobs, uint32_t* d_ntx, hipStream_t st);
hipError_t launch_notary_tx(const uint8_t* d_bodies, const uint64_t* d_off, const void* d_blobs,
                            const uint32_t* d_ntx, uint32_t n_shards, uint32_t max_txs, const uint8_t* d_cid64,
                            const uint8_t* d_suffix, uint32_t slen, int signer_kind, const uint4* gtab,
                            uint8_t* d_bitmap, uint32_t bm_bytes, uint8_t* d_senders, uint8_t* d_status,
                            hipStream_t st);
hipError_t launch_notary_synth(uint64_t seed, uint32_t shard0, uint32_t n_shards, uint32_t txs_per_shard,
                               const uint4* gtab, uint8_t* d_bodies, uint8_t* d_exp_status, uint8_t* d_exp_sender,
                               hipStream_t st);

// fixed-base comb for u1*G: ceil(256 / COMB_BITS) windows of 2^COMB_BITS affine entries d * 2^(COMB_BITS w) * G.
// 20-bit windows: 13 mixed adds per u1*G over a 1.09 GB table in HBM (one random 80-byte read per
// window, prefetched a window ahead); 16-bit: 16 adds, 80 MiB (Infinity-Cache resident), 1.3 % slower;
// 22-bit: 12 adds, 4 GB, within 0.1 % of 20-bit (profiles/r02/ab_comb.txt).  The table is built once
// per context (k_gtable_base + k_gtable_init).
constexpr int COMB_BITS = 20;
constexpr int COMB_WINDOWS = (256 + COMB_BITS - 1) / COMB_BITS;  // the top window may be partial
static_assert(COMB_BITS >= 4 && COMB_BITS <= 26, "comb window width");
constexpr size_t GTAB_ENTRIES = (size_t)COMB_WINDOWS << COMB_BITS;
constexpr size_t GTAB_ENTRY_BYTES = 80;  // fe9 x[9] y[9] + 2 pad words (secp256k1_comb.cuh gtab_load)
constexpr size_t GTAB_BYTES = GTAB_ENTRIES * GTAB_ENTRY_BYTES;

// signatures whose r a lane of k_rinv_batch inverts with one safegcd inversion (secp256k1_rinv.cuh):
// 16 makes a batch of 2^20 one wave per SIMD (measured against 8 and 32: profiles/r11/README.md)
#ifndef GSV_RINV_K
#define GSV_RINV_K 16
#endif
constexpr int RINV_K = GSV_RINV_K;
static_assert(RINV_K >= 1 && RINV_K <= 64, "r values per inversion");

}  // namespace gsv

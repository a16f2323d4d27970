// Size arithmetic of one device allocation, free of HIP (plain C++17; tests/native/staging_host.cpp
// compiles it with g++).  A Layout collects 256-B aligned regions first and is bound to memory
// afterwards: a prepared shape's workspace (Shape::at) and the buffers a host-pointer entry point
// stages in the context's arena.  Every staged buffer is declared once, in the *Stage struct of its
// entry point; the total to reserve is the Layout's `n` after those declarations.  A pointer exists only once
// the arena is reserved, and is bound after the call's last reservation (arena_reserve may move the arena):
// the host forms bind through their Staged (gsv_ctx.h), s(buf), which also copies no more into or out of a
// buffer than the `bytes` declared here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gsv {
namespace api {

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

constexpr size_t kAbsent = ~(size_t)0;

// a staged buffer: its offset in the allocation, or absent (an optional output the caller did not ask
// for: reserves nothing, binds to nullptr)
template <typename T>
struct Buf {
    size_t off = kAbsent, bytes = 0;
    T* operator()(uint8_t* base) const { return off == kAbsent ? nullptr : (T*)(base + off); }
};

// regions of one device allocation (256-B aligned offsets; a zero-length region still gets 256 B, so
// no two regions share an address)
struct Layout {
    size_t n = 0;
    size_t add(size_t bytes) {
        size_t o = n;
        n += al(bytes ? bytes : 1);
        return o;
    }
    template <typename T = uint8_t>
    Buf<T> buf(size_t bytes, bool present = true) {
        return present ? Buf<T>{add(bytes), bytes} : Buf<T>{};
    }
};

using B8 = Buf<uint8_t>;

// ---- the staged buffers of the host-pointer entry points (in arena order)
struct KeccakStage {  // gsv_keccak256_batch
    B8 data;
    Buf<uint64_t> off;
    B8 out;
    KeccakStage(Layout& L, size_t bytes, size_t n)
        : data(L.buf(bytes + 8)), off(L.buf<uint64_t>((n + 1) * 8)), out(L.buf(n * 32)) {}
};
struct EcrecoverStage {  // gsv_ecrecover_batch
    B8 msg, sig, pub, addr, st;
    EcrecoverStage(Layout& L, size_t n, bool want_pub, bool want_addr)
        : msg(L.buf(n * 32)), sig(L.buf(n * 65)), pub(L.buf(n * 65, want_pub)), addr(L.buf(n * 20, want_addr)),
          st(L.buf(n)) {}
};
struct VerifyStage {  // gsv_ecdsa_verify_batch: keys in the device layout (pubkey_pack.h)
    B8 msg, sig, pub, len, ok;
    VerifyStage(Layout& L, size_t n)
        : msg(L.buf(n * 32)), sig(L.buf(n * 64)), pub(L.buf(n * 65)), len(L.buf(n)), ok(L.buf(n)) {}
};
struct PubkeyParseStage {  // gsv_pubkey_parse_batch
    B8 pub, len, out, ok;
    PubkeyParseStage(Layout& L, size_t n) : pub(L.buf(n * 65)), len(L.buf(n)), out(L.buf(n * 65)), ok(L.buf(n)) {}
};
// gsv_ecdsa_sign_batch, gsv_pubkey_create_batch.  The secret keys come FIRST, so the region the host
// form overwrites before it returns is [key.off, key.off + key.bytes) whatever else is staged.
struct SignStage {
    B8 key, msg, sig, st;
    SignStage(Layout& L, size_t n) : key(L.buf(n * 32)), msg(L.buf(n * 32)), sig(L.buf(n * 65)), st(L.buf(n)) {}
};
struct PubkeyCreateStage {
    B8 key, pub, addr, st;
    PubkeyCreateStage(Layout& L, size_t n, bool want_addr)
        : key(L.buf(n * 32)), pub(L.buf(n * 65)), addr(L.buf(n * 20, want_addr)), st(L.buf(n)) {}
};
// gsv_tx_sign_batch.  The secret keys come FIRST, as in SignStage.  `work` is work_per bytes per item
// (gsv_tx_sign_work_bytes); `out` holds the slots: the input's bytes plus `growth` per item.
struct TxSignStage {
    B8 key, work, rlp;
    Buf<uint64_t> off;
    B8 out;
    Buf<uint32_t> olen;
    B8 hash, st;
    TxSignStage(Layout& L, size_t n, size_t work_per, size_t bytes, size_t growth, bool want_hash)
        : key(L.buf(n * 32)), work(L.buf(n * work_per)), rlp(L.buf(bytes + 8)), off(L.buf<uint64_t>((n + 1) * 8)),
          out(L.buf(bytes + n * growth)), olen(L.buf<uint32_t>(n * 4)), hash(L.buf(n * 32, want_hash)), st(L.buf(n)) {}
};
// gsv_secp256k1_scalar_mul_batch, gsv_ecdh_batch.  Every secret region comes FIRST and contiguous: the
// scalars, then the secret outputs (the product point; the shared X and the derived keys, each only
// when asked for).  `secret` is the end of the last of them: the host form overwrites [0, secret) of
// the stage before it returns, whatever else is staged behind (the public points, the status bytes).
struct ScalarMulStage {
    B8 key, out;
    size_t secret;
    B8 pt, st;
    ScalarMulStage(Layout& L, size_t n)
        : key(L.buf(n * 32)), out(L.buf(n * 64)), secret(L.n), pt(L.buf(n * 64)), st(L.buf(n)) {}
};
struct EcdhStage {
    B8 key, shared, keys;
    size_t secret;
    B8 pt, st;
    EcdhStage(Layout& L, size_t n, bool want_shared, bool want_keys)
        : key(L.buf(n * 32)), shared(L.buf(n * 32, want_shared)), keys(L.buf(n * 48, want_keys)), secret(L.n),
          pt(L.buf(n * 64)), st(L.buf(n)) {}
};
// gsv_ecies_decrypt_batch, gsv_ecies_encrypt_batch.  The same rule: the secret (or ephemeral) keys, the
// work area the launches share (Ke || Km) and the plaintext (Decrypt's output, Encrypt's input) come
// FIRST and contiguous, `secret` is their end, and the host form overwrites [0, secret).  `work` is
// work_per bytes per item (gsv_ecies_work_bytes); s2 and its offset table are absent when the caller
// passes none.
struct EciesDecryptStage {
    B8 key, work, msg;
    size_t secret;
    B8 ct;
    Buf<uint64_t> off;
    B8 s2;
    Buf<uint64_t> s2off;
    Buf<uint32_t> mlen;
    B8 st;
    EciesDecryptStage(Layout& L, size_t n, size_t work_per, size_t bytes, size_t s2_bytes, bool has_s2)
        : key(L.buf(n * 32)), work(L.buf(n * work_per)), msg(L.buf(bytes)), secret(L.n), ct(L.buf(bytes)),
          off(L.buf<uint64_t>((n + 1) * 8)), s2(L.buf(s2_bytes, has_s2)), s2off(L.buf<uint64_t>((n + 1) * 8, has_s2)),
          mlen(L.buf<uint32_t>(n * 4)), st(L.buf(n)) {}
};
struct EciesEncryptStage {
    B8 key, work, msg;
    size_t secret;
    B8 pub, iv;
    Buf<uint64_t> off;
    B8 s2;
    Buf<uint64_t> s2off;
    B8 ct, st;
    EciesEncryptStage(Layout& L, size_t n, size_t work_per, size_t bytes, size_t s2_bytes, bool has_s2)
        : key(L.buf(n * 32)), work(L.buf(n * work_per)), msg(L.buf(bytes)), secret(L.n), pub(L.buf(n * 64)),
          iv(L.buf(n * 16)), off(L.buf<uint64_t>((n + 1) * 8)), s2(L.buf(s2_bytes, has_s2)),
          s2off(L.buf<uint64_t>((n + 1) * 8, has_s2)), ct(L.buf(bytes + n * 113)), st(L.buf(n)) {}
};
// fixed-size records in, fixed-size results and a status byte out: gsv_ecrecover_precompile_batch
// (128 -> 32), bn_g1_host (128 or 96 -> 64)
struct RecordStage {
    B8 in, out, st;
    RecordStage(Layout& L, size_t n, size_t rec, size_t res) : in(L.buf(n * rec)), out(L.buf(n * res)), st(L.buf(n)) {}
};
// gsv_modexp_batch, once per width class: the rows base || exp || mod of the class's items, their
// results, and the device form's work buffer (gsv_modexp_work_bytes; none for the 32-byte class)
struct ModexpStage {
    B8 in, out, work;
    ModexpStage(Layout& L, size_t in_bytes, size_t out_bytes, size_t work_bytes)
        : in(L.buf(in_bytes)), out(L.buf(out_bytes)), work(L.buf(work_bytes, work_bytes != 0)) {}
};
struct SenderStage {  // gsv_sender_batch, and the tail of tx_sender_impl
    B8 h, r, s;
    Buf<uint64_t> v;
    B8 vb, a, st;
    SenderStage(Layout& L, size_t n)
        : h(L.buf(n * 32)), r(L.buf(n * 32)), s(L.buf(n * 32)), v(L.buf<uint64_t>(n * 8)), vb(L.buf(n)),
          a(L.buf(n * 20)), st(L.buf(n)) {}
};
struct TxSenderStage {  // tx_sender_impl: the sighash preimages, then recoverPlain's buffers
    B8 pre;
    Buf<uint64_t> poff;
    SenderStage snd;
    TxSenderStage(Layout& L, size_t pbytes, size_t n)
        : pre(L.buf(pbytes + 8)), poff(L.buf<uint64_t>((n + 1) * 8)), snd(L, n) {}
};
struct SynthSignStage {  // gsv_synth_sign
    B8 msg, sig, pub, addr;
    SynthSignStage(Layout& L, size_t n, bool want_pub, bool want_addr)
        : msg(L.buf(n * 32)), sig(L.buf(n * 65)), pub(L.buf(n * 65, want_pub)), addr(L.buf(n * 20, want_addr)) {}
};
// `bytes` of bodies (16-byte aligned starts, stage_offsets) or list values in, a root per body or list
// out: gsv_chunk_root_batch, gsv_collation_poc_batch, gsv_derive_sha_batch
struct RootsStage {
    B8 in, roots;
    RootsStage(Layout& L, size_t bytes, size_t n) : in(L.buf(bytes + 16)), roots(L.buf(n * 32)) {}
};
struct PairingStage {  // gsv_bn256_pairing_check_batch
    B8 in, verdict;
    PairingStage(Layout& L, size_t bytes, size_t n) : in(L.buf(bytes + 8)), verdict(L.buf(n)) {}
};
// gsv_notary_validate_shards, and the rank's own block in gsv_notary_validate_partition
struct NotaryStage {
    B8 bodies, root;
    Buf<uint32_t> ntx;
    B8 bitmap, senders, status;
    NotaryStage(Layout& L, size_t bytes, size_t n, uint32_t max_txs, bool want_senders, bool want_status)
        : bodies(L.buf(bytes + 16)), root(L.buf(n * 32)), ntx(L.buf<uint32_t>(n * 4)),
          bitmap(L.buf(n * ((max_txs + 7) / 8))), senders(L.buf(n * max_txs * 20, want_senders)),
          status(L.buf(n * max_txs, want_status)) {}
};

// shard partition: rank r of N validates shards [first, first + n) of n_total; a block is a header
// {int32 status, uint32 shards} + `per` records of R bytes
struct PartDims {
    size_t first, n, per, R, bm, B;
};
inline PartDims part_dims(size_t n_total, int N, int r, uint32_t max_txs) {
    PartDims d;
    d.first = n_total * (size_t)r / (size_t)N;
    d.n = n_total * (size_t)(r + 1) / (size_t)N - d.first;
    d.per = (n_total + N - 1) / N;
    d.bm = (max_txs + 7) / 8;
    d.R = (36 + d.bm + 7) / 8 * 8;  // root 32 | ntx 4 | bitmap, padded to 8 (gsv/shards.py)
    d.B = 8 + d.per * d.R;          // header {int32 status, uint32 shards} + records
    return d;
}
// gsv_notary_validate_partition: the rank's block, the gathered blocks, the gathered outputs and the
// per-rank status words come FIRST (`gathered` = their end), so a rank whose own block failed reserves
// only those and still joins the all-gather; the own block's buffers follow
struct PartitionStage {
    B8 blk, all, oroot;
    Buf<uint32_t> ontx;
    B8 obm;
    Buf<int32_t> rst;
    size_t gathered;
    NotaryStage own;
    PartitionStage(Layout& L, const PartDims& d, size_t n_total, int N, size_t bytes, uint32_t max_txs,
                   bool want_senders, bool want_status)
        : blk(L.buf(d.B)), all(L.buf((size_t)N * d.B)), oroot(L.buf(n_total * 32)),
          ontx(L.buf<uint32_t>(n_total * 4)), obm(L.buf(n_total * d.bm)), rst(L.buf<int32_t>((size_t)N * 4)),
          gathered(L.n), own(L, bytes, d.n, max_txs, want_senders, want_status) {}
};
struct BlobSerStage {  // gsv_blob_serialize_batch
    B8 blobs, skip, bodies;
    BlobSerStage(Layout& L, size_t blob_bytes, size_t nblobs, bool has_skip, size_t body_bytes)
        : blobs(L.buf(blob_bytes)), skip(L.buf(nblobs, has_skip)), bodies(L.buf(body_bytes)) {}
};
struct BlobDeserStage {  // gsv_blob_deserialize_batch
    B8 bodies;
    Buf<uint32_t> nblobs, start, len;
    B8 skip, data;
    BlobDeserStage(Layout& L, size_t body_bytes, size_t n, uint32_t max_blobs, size_t data_bytes)
        : bodies(L.buf(body_bytes)), nblobs(L.buf<uint32_t>(n * 4)), start(L.buf<uint32_t>(n * max_blobs * 4)),
          len(L.buf<uint32_t>(n * max_blobs * 4)), skip(L.buf(n * max_blobs)), data(L.buf(data_bytes)) {}
};
// gsv_proposer_create_collations.  The secret keys come FIRST, as in SignStage: the region the host
// form overwrites before it returns is [key.off, key.off + key.bytes).
struct ProposerStage {
    B8 key, blobs, sid, per, prop, bodies, root, hash, sig, st;
    ProposerStage(Layout& L, size_t n, size_t blob_bytes, size_t body_bytes)
        : key(L.buf(n * 32)), blobs(L.buf(blob_bytes)), sid(L.buf(n * 32)), per(L.buf(n * 32)), prop(L.buf(n * 20)),
          bodies(L.buf(body_bytes)), root(L.buf(n * 32)), hash(L.buf(n * 32)), sig(L.buf(n * 65)), st(L.buf(n)) {}
};
struct HeaderStage {  // gsv_collation_header_verify_batch
    B8 sid, root, per, prop, sig, nil, hash, signer, st, scr;
    HeaderStage(Layout& L, size_t n, size_t scratch_bytes, bool has_nil, bool want_hash, bool want_signer)
        : sid(L.buf(n * 32)), root(L.buf(n * 32)), per(L.buf(n * 32)), prop(L.buf(n * 20)), sig(L.buf(n * 65)),
          nil(L.buf(n, has_nil)), hash(L.buf(n * 32, want_hash)), signer(L.buf(n * 20, want_signer)), st(L.buf(n)),
          scr(L.buf(scratch_bytes)) {}
};
// gsv_ethash_light_batch / gsv_ethash_verify_seal_batch, one epoch's items: a and b are the two 32-byte
// outputs (mix digest, result) or the two 32-byte inputs (mix digest, difficulty) of the verify form
struct EthashStage {
    B8 hash;
    Buf<uint64_t> nonce;
    B8 a, b, st;
    EthashStage(Layout& L, size_t n, bool verify)
        : hash(L.buf(n * 32)), nonce(L.buf<uint64_t>(n * 8)), a(L.buf(n * 32)), b(L.buf(n * 32)),
          st(L.buf(n, verify)) {}
};
// gsv_ethash_seal_batch, one round's slice of headers: what gsv_ethash_search_dev reads and writes
struct EthashSealStage {
    B8 hash, diff;
    Buf<uint64_t> start, nonce;
    Buf<uint32_t> offset;
    B8 mix, result, found;
    EthashSealStage(Layout& L, size_t n)
        : hash(L.buf(n * 32)), diff(L.buf(n * 32)), start(L.buf<uint64_t>(n * 8)), nonce(L.buf<uint64_t>(n * 8)),
          offset(L.buf<uint32_t>(n * 4)), mix(L.buf(n * 32)), result(L.buf(n * 32)), found(L.buf(n)) {}
};
// gsv_block_header_hash_batch, gsv_calc_difficulty_batch, gsv_ethash_verify_headers_batch: the items (and the
// parent of header 0), the records (`work`, bh::work_bytes(n)) and what the launches write.  `time` is the
// difficulty form's input; hnn .. diff are the arrays the seal call takes; pre is the decode status of the
// hash and difficulty forms.
struct BlockHeaderStage {
    B8 rlp;
    Buf<uint64_t> off;
    B8 parent, work, hash, hnn;
    Buf<uint64_t> nonce, number, time;
    B8 mix, diff, want, pre, post;
    BlockHeaderStage(Layout& L, size_t bytes, size_t n, size_t parent_len, size_t work_bytes, bool rules, bool calc)
        : rlp(L.buf(bytes + 8)), off(L.buf<uint64_t>((n + 1) * 8)), parent(L.buf(parent_len + 8, parent_len != 0)),
          work(L.buf(work_bytes)), hash(L.buf(n * 32, !calc)), hnn(L.buf(n * 32, !calc)),
          nonce(L.buf<uint64_t>(n * 8, rules)), number(L.buf<uint64_t>(n * 8, rules)),
          time(L.buf<uint64_t>(n * 8, calc)), mix(L.buf(n * 32, rules)), diff(L.buf(n * 32, rules)),
          want(L.buf(n * 32, rules || calc)), pre(L.buf(n)), post(L.buf(n, rules)) {}
};
// the last step of gsv_ethash_verify_headers_batch, staged again behind the ethash path's own use of the
// arena: the three statuses of each header in, the merged one out
struct BlockMergeStage {
    B8 pre, seal, post, out;
    BlockMergeStage(Layout& L, size_t n) : pre(L.buf(n)), seal(L.buf(n)), post(L.buf(n)), out(L.buf(n)) {}
};
// gsv_bloom9_batch: the messages and their rebased table in, three bit numbers per message out
struct Bloom9Stage {
    B8 data;
    Buf<uint64_t> off;
    Buf<uint16_t> idx;
    Bloom9Stage(Layout& L, size_t bytes, size_t n)
        : data(L.buf(bytes + 8)), off(L.buf<uint64_t>((n + 1) * 8)), idx(L.buf<uint16_t>(n * 6)) {}
};
// gsv_receipts_verify_batch: the receipts' bytes and both rebased tables, the work area of the _dev chain
// (gsv_receipts_work_bytes), what the chain writes, and the header's three values where the caller gave them
struct ReceiptStage {
    B8 vals;
    Buf<uint64_t> voff, loff;
    B8 work, rstatus, lbloom, roots;
    Buf<uint64_t> gas;
    B8 lstatus, status, want_bloom, want_root;
    Buf<uint64_t> want_gas;
    ReceiptStage(Layout& L, size_t bytes, size_t n, size_t n_lists, size_t work_bytes, bool has_bloom, bool has_root,
                 bool has_gas)
        : vals(L.buf(bytes + 16)), voff(L.buf<uint64_t>((n + 1) * 8)), loff(L.buf<uint64_t>((n_lists + 1) * 8)),
          work(L.buf(work_bytes)), rstatus(L.buf(n)), lbloom(L.buf(n_lists * 256)), roots(L.buf(n_lists * 32)),
          gas(L.buf<uint64_t>(n_lists * 8)), lstatus(L.buf(n_lists)), status(L.buf(n_lists)),
          want_bloom(L.buf(n_lists * 256, has_bloom)), want_root(L.buf(n_lists * 32, has_root)),
          want_gas(L.buf<uint64_t>(n_lists * 8, has_gas)) {}
};
// gsv_bloombits_generate_batch: the sections' blooms in, the table out
struct BloombitsGenerateStage {
    B8 blooms, bits;
    BloombitsGenerateStage(Layout& L, size_t bloom_bytes, size_t table_bytes)
        : blooms(L.buf(bloom_bytes)), bits(L.buf(table_bytes)) {}
};
// gsv_bitset_compress_batch: n vectors of `len` bytes in; their slots and lengths out
struct BitsetCompressStage {
    B8 in, slots;
    Buf<uint32_t> len;
    BitsetCompressStage(Layout& L, size_t n, size_t len_)
        : in(L.buf(n * len_)), slots(L.buf(n * len_)), len(L.buf<uint32_t>(n * 4)) {}
};
// gsv_bitset_decompress_batch: the packed inputs and their rebased table in; n rows of `len` bytes and a status out
struct BitsetDecompressStage {
    B8 data;
    Buf<uint64_t> off;
    B8 out, st;
    BitsetDecompressStage(Layout& L, size_t bytes, size_t n, size_t len)
        : data(L.buf(bytes + 8)), off(L.buf<uint64_t>((n + 1) * 8)), out(L.buf(n * len)), st(L.buf(n)) {}
};
// the filter system of gsv_bloombits_match_batch and gsv_bloom_filter_batch: the kept clauses' bytes and their table
// (what bloom9 hashes), the three bit numbers of each, and the two tables of the rules that remain
struct FilterStage {
    B8 data;
    Buf<uint64_t> off;
    Buf<uint16_t> idx;
    Buf<uint32_t> rule_off, query_off;
    FilterStage(Layout& L, size_t bytes, size_t n_clauses, size_t n_rules, size_t n_queries)
        : data(L.buf(bytes + 8)), off(L.buf<uint64_t>((n_clauses + 1) * 8)), idx(L.buf<uint16_t>(n_clauses * 6)),
          rule_off(L.buf<uint32_t>((n_rules + 1) * 4)), query_off(L.buf<uint32_t>((n_queries + 1) * 4)) {}
};
// gsv_bloombits_match_batch: the filter, the table and the ranges in; the match bitsets and counts between the
// launches; the scanned totals and the block numbers out
struct BloombitsMatchStage {
    FilterStage f;
    B8 bits;
    Buf<uint64_t> begin, end;
    B8 match;
    Buf<uint32_t> count;
    Buf<uint64_t> block_off, blocks;
    BloombitsMatchStage(Layout& L, size_t clause_bytes, size_t n_clauses, size_t n_rules, size_t n_queries,
                        size_t table_bytes, size_t match_bytes, size_t pairs, size_t capacity)
        : f(L, clause_bytes, n_clauses, n_rules, n_queries), bits(L.buf(table_bytes)),
          begin(L.buf<uint64_t>(n_queries * 8)), end(L.buf<uint64_t>(n_queries * 8)), match(L.buf(match_bytes)),
          count(L.buf<uint32_t>(pairs * 4)), block_off(L.buf<uint64_t>((n_queries + 1) * 8)),
          blocks(L.buf<uint64_t>(capacity * 8)) {}
};
// gsv_bloom_filter_batch: the filter and the blooms in, a byte per (query, bloom) out
struct BloomFilterStage {
    FilterStage f;
    B8 blooms, out;
    BloomFilterStage(Layout& L, size_t clause_bytes, size_t n_clauses, size_t n_rules, size_t n_queries, size_t n_blooms)
        : f(L, clause_bytes, n_clauses, n_rules, n_queries), blooms(L.buf(n_blooms * 256)),
          out(L.buf(n_queries * n_blooms)) {}
};

}  // namespace api
}  // namespace gsv

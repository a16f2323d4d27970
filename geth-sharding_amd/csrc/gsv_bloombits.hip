// The bloombits family of the C ABI (gsv_ctx.h): the device forms check their arguments and enqueue launches of
// bloombits.hip; the host forms stage, run them and copy back.  The two filter forms first reduce the filter system
// the way NewMatcher does (bloombits_host.h) and hash the clauses that remain with the bloom9 kernel.
#include "bloombits_host.h"
#include "gsv_ctx.h"

using namespace gsv::api;
namespace bb = gsv::bb;

namespace {

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

constexpr uint64_t kMaxFirstSection = 1ull << 40;  // (first_section + n_sections) * S stays far below 2^64

// A host filter system reduced to what NewMatcher keeps: the tables over the kept rules and clauses, and the kept
// clauses' bytes packed behind a table that starts at 0 (what bloom9 hashes).
struct HostFilter {
    bb::Filters f;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
    size_t n_clauses() const { return f.clause.size(); }
    size_t n_rules() const { return f.rule_off.size() - 1; }
};

int host_filter(const uint8_t* clause_data, const uint64_t* clause_off, const uint8_t* clause_nil,
                const uint64_t* rule_off, const uint64_t* query_off, size_t n_queries, HostFilter& h) {
    if (!query_off) return GSV_E_INVALID_ARG;
    GSVCHK(table_order(query_off, n_queries));
    const uint64_t n_rules = query_off[n_queries] - query_off[0];
    if (n_rules > bb::MAX_RULES || (n_rules && !rule_off)) return GSV_E_INVALID_ARG;
    uint64_t n_clauses = 0;
    if (n_rules) {
        const uint64_t* ro = rule_off + query_off[0];
        GSVCHK(table_order(ro, n_rules));
        n_clauses = ro[n_rules] - ro[0];
        if (n_clauses > bb::MAX_CLAUSES || (n_clauses && !clause_off)) return GSV_E_INVALID_ARG;
        if (n_clauses) GSVCHK(table_check(clause_data, clause_off + ro[0], n_clauses));
    }
    if (!bb::drop_rules(query_off, n_queries, rule_off, clause_nil, h.f)) return GSV_E_INVALID_ARG;
    h.off.assign(1, 0);
    h.bytes.clear();
    for (uint64_t c : h.f.clause) {
        h.bytes.insert(h.bytes.end(), clause_data + clause_off[c], clause_data + clause_off[c + 1]);
        h.off.push_back(h.bytes.size());
    }
    return GSV_SUCCESS;
}

// the filter staged and its clauses hashed on the context's stream
int stage_filter(gsv_ctx* c, Staged& s, const FilterStage& p, const HostFilter& h) {
    GSVCHK(s.in(p.data, h.bytes.data(), h.bytes.size()));
    GSVCHK(s.in(p.off, h.off.data()));
    GSVCHK(s.in(p.rule_off, h.f.rule_off.data()));
    GSVCHK(s.in(p.query_off, h.f.query_off.data()));
    return gsv_bloom9_batch_dev(c, s(p.data), s(p.off), h.n_clauses(), s(p.idx), c->stream);
}

bool filter_args_ok(const uint16_t* d_clauses, size_t n_clauses, const uint32_t* d_rule_off, size_t n_rules,
                    const uint32_t* d_query_off, size_t n_queries) {
    if (n_queries > bb::MAX_QUERIES || n_rules > bb::MAX_RULES || n_clauses > bb::MAX_CLAUSES) return false;
    if (!d_query_off || !aligned(d_query_off, 4)) return false;
    if (n_rules && (!d_rule_off || !aligned(d_rule_off, 4))) return false;
    if (n_clauses && (!d_clauses || !aligned(d_clauses, 2))) return false;
    return true;
}

}  // namespace

extern "C" {

int gsv_bloombits_generate_dev(gsv_ctx* c, const uint8_t* d_blooms256, size_t n_sections, uint32_t section_size,
                               uint8_t* d_bits, void* stream) {
    if (!c || !bb::section_ok(section_size) || n_sections > bb::MAX_SECTIONS) return GSV_E_INVALID_ARG;
    if (n_sections == 0) return GSV_SUCCESS;
    if (!d_blooms256 || !d_bits) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BLOOMBITS_GENERATE, st);
    return hip_err(gsv::launch_bloombits_generate(d_blooms256, (uint32_t)n_sections, section_size, d_bits, st));
}

int gsv_bloombits_generate_batch(gsv_ctx* c, const uint8_t* blooms256, size_t n_sections, uint32_t section_size,
                                 uint8_t* bits_out) {
    if (!c || !bb::section_ok(section_size) || n_sections > bb::MAX_SECTIONS) return GSV_E_INVALID_ARG;
    if (n_sections == 0) return GSV_SUCCESS;
    if (!blooms256 || !bits_out) return GSV_E_INVALID_ARG;
    Layout L;
    const BloombitsGenerateStage p(L, bb::blooms_bytes(n_sections, section_size), bb::table_bytes(n_sections, section_size));
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.blooms, blooms256));
    GSVCHK(gsv_bloombits_generate_dev(c, s(p.blooms), n_sections, section_size, s(p.bits), c->stream));
    GSVCHK(s.out(bits_out, p.bits));
    return s.finish();
}

int gsv_bitset_compress_batch_dev(gsv_ctx* c, const uint8_t* d_in, size_t n, uint32_t len, uint8_t* d_slots,
                                  uint32_t* d_len, void* stream) {
    if (!c || len < 1 || len > bb::MAX_VECTOR || n > bb::MAX_VECTORS) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!d_in || !d_slots || !d_len || !aligned(d_len, 4)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BITSET_COMPRESS, st);
    return hip_err(gsv::launch_bitset_compress(d_in, (uint32_t)n, len, d_slots, d_len, st));
}

int gsv_bitset_compress_batch(gsv_ctx* c, const uint8_t* in, size_t n, uint32_t len, uint8_t* out, uint64_t* out_off) {
    if (!c || len < 1 || len > bb::MAX_VECTOR || n > bb::MAX_VECTORS) return GSV_E_INVALID_ARG;
    if (n == 0) {
        if (out_off) out_off[0] = 0;
        return GSV_SUCCESS;
    }
    if (!in || !out || !out_off) return GSV_E_INVALID_ARG;
    Layout L;
    const BitsetCompressStage p(L, n, len);
    std::vector<uint32_t> lens(n);
    {
        Staged s(c, L);
        if (s.rc) return s.rc;
        GSVCHK(s.in(p.in, in));
        GSVCHK(gsv_bitset_compress_batch_dev(c, s(p.in), n, len, s(p.slots), s(p.len), c->stream));
        GSVCHK(s.out(lens.data(), p.len));
        GSVCHK(s.out(out, p.slots));
        GSVCHK(s.finish());
    }
    // the slots packed towards the front of `out`; what lay behind a slot's length was never written by the
    // kernel, so nothing behind the packed bytes is handed on
    if (!bb::pack_slots(out, lens.data(), n, len, out, out_off)) return GSV_E_HIP;
    memset(out + out_off[n], 0, n * (size_t)len - out_off[n]);
    return GSV_SUCCESS;
}

int gsv_bitset_decompress_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n, uint32_t len,
                                    uint8_t* d_out, uint8_t* d_status, void* stream) {
    if (!c || len < 1 || len > bb::MAX_VECTOR || n > bb::MAX_VECTORS) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!d_off || !aligned(d_off, 8) || !d_out || !d_status) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BITSET_DECOMPRESS, st);
    return hip_err(gsv::launch_bitset_decompress(d_data, d_off, (uint32_t)n, len, d_out, d_status, st));
}

int gsv_bitset_decompress_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n, uint32_t len,
                                uint8_t* out, uint8_t* status) {
    if (!c || len < 1 || len > bb::MAX_VECTOR || n > bb::MAX_VECTORS) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!off || !out || !status) return GSV_E_INVALID_ARG;
    GSVCHK(table_check(data, off, n));
    const size_t bytes = off[n] - off[0];
    const std::vector<uint64_t> rel = table_rebase(off, n);
    Layout L;
    const BitsetDecompressStage p(L, bytes, n, len);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.data, data + off[0], bytes));
    GSVCHK(s.in(p.off, rel.data()));
    GSVCHK(gsv_bitset_decompress_batch_dev(c, s(p.data), s(p.off), n, len, s(p.out), s(p.st), c->stream));
    GSVCHK(s.out(out, p.out));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

int gsv_bloombits_match_dev(gsv_ctx* c, const uint8_t* d_bits, uint32_t section_size, uint64_t first_section,
                            size_t n_sections, const uint16_t* d_clauses, size_t n_clauses, const uint32_t* d_rule_off,
                            size_t n_rules, const uint32_t* d_query_off, size_t n_queries, const uint64_t* d_begin,
                            const uint64_t* d_end, uint8_t* d_match, uint32_t* d_count, void* stream) {
    if (!c || !bb::section_ok(section_size) || !bb::pairs_ok(n_queries, n_sections) || first_section > kMaxFirstSection)
        return GSV_E_INVALID_ARG;
    if (n_queries == 0 || n_sections == 0) return GSV_SUCCESS;
    if (!filter_args_ok(d_clauses, n_clauses, d_rule_off, n_rules, d_query_off, n_queries)) return GSV_E_INVALID_ARG;
    if (!d_bits || !d_begin || !aligned(d_begin, 8) || !d_end || !aligned(d_end, 8) || !d_match || !d_count ||
        !aligned(d_count, 4))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BLOOMBITS_MATCH, st);
    return hip_err(gsv::launch_bloombits_match(d_bits, section_size, first_section, (uint32_t)n_sections, d_clauses,
                                               (uint32_t)n_clauses, d_rule_off, (uint32_t)n_rules, d_query_off,
                                               (uint32_t)n_queries, d_begin, d_end, d_match, d_count, st));
}

int gsv_bloombits_blocks_dev(gsv_ctx* c, const uint8_t* d_match, const uint32_t* d_count, uint32_t section_size,
                             uint64_t first_section, size_t n_sections, size_t n_queries, uint64_t* d_block_off,
                             uint64_t* d_blocks, uint64_t capacity, void* stream) {
    if (!c || !bb::section_ok(section_size) || !bb::pairs_ok(n_queries, n_sections) || first_section > kMaxFirstSection)
        return GSV_E_INVALID_ARG;
    if (n_queries == 0) return GSV_SUCCESS;
    if (!d_block_off || !aligned(d_block_off, 8) || (capacity && (!d_blocks || !aligned(d_blocks, 8))))
        return GSV_E_INVALID_ARG;
    if (n_sections && (!d_match || !d_count || !aligned(d_count, 4))) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    {
        KTimer t(c, GSV_K_BLOOMBITS_TOTALS, st);
        HIPCHK(gsv::launch_bloombits_totals(d_count, (uint32_t)n_sections, (uint32_t)n_queries, d_block_off, st));
    }
    {
        KTimer t(c, GSV_K_BLOOMBITS_SCAN, st);
        HIPCHK(gsv::launch_bloombits_scan(d_block_off, (uint32_t)n_queries, st));
    }
    if (n_sections == 0) return GSV_SUCCESS;
    KTimer t(c, GSV_K_BLOOMBITS_BLOCKS, st);
    return hip_err(gsv::launch_bloombits_blocks(d_match, d_count, section_size, first_section, (uint32_t)n_sections,
                                                (uint32_t)n_queries, d_block_off, d_blocks, capacity, st));
}

int gsv_bloombits_match_batch(gsv_ctx* c, const uint8_t* bits, uint32_t section_size, uint64_t first_section,
                              size_t n_sections, const uint8_t* clause_data, const uint64_t* clause_off,
                              const uint8_t* clause_nil, const uint64_t* rule_off, const uint64_t* query_off,
                              size_t n_queries, const uint64_t* begin, const uint64_t* end, uint64_t* block_off_out,
                              uint64_t* blocks_out, uint64_t capacity) {
    if (!c || !bb::section_ok(section_size) || !bb::pairs_ok(n_queries, n_sections) || first_section > kMaxFirstSection ||
        capacity > (1ull << 40))
        return GSV_E_INVALID_ARG;
    if (n_queries == 0) {
        if (block_off_out) block_off_out[0] = 0;
        return GSV_SUCCESS;
    }
    if (!begin || !end || !block_off_out || (capacity && !blocks_out) || (n_sections && !bits)) return GSV_E_INVALID_ARG;
    HostFilter h;
    GSVCHK(host_filter(clause_data, clause_off, clause_nil, rule_off, query_off, n_queries, h));
    Layout L;
    const BloombitsMatchStage p(L, h.bytes.size(), h.n_clauses(), h.n_rules(), n_queries,
                                bb::table_bytes(n_sections, section_size),
                                bb::match_bytes(n_queries, n_sections, section_size), n_queries * n_sections, capacity);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(stage_filter(c, s, p.f, h));
    if (n_sections) GSVCHK(s.in(p.bits, bits));
    GSVCHK(s.in(p.begin, begin));
    GSVCHK(s.in(p.end, end));
    GSVCHK(gsv_bloombits_match_dev(c, s(p.bits), section_size, first_section, n_sections, s(p.f.idx), h.n_clauses(),
                                   s(p.f.rule_off), h.n_rules(), s(p.f.query_off), n_queries, s(p.begin), s(p.end),
                                   s(p.match), s(p.count), c->stream));
    GSVCHK(gsv_bloombits_blocks_dev(c, s(p.match), s(p.count), section_size, first_section, n_sections, n_queries,
                                    s(p.block_off), s(p.blocks), capacity, c->stream));
    GSVCHK(s.out(block_off_out, p.block_off));
    GSVCHK(s.finish());
    const uint64_t got = std::min<uint64_t>(block_off_out[n_queries], capacity);
    GSVCHK(s.out(blocks_out, p.blocks, (size_t)got * 8));
    return s.finish();
}

int gsv_bloom_filter_dev(gsv_ctx* c, const uint8_t* d_blooms256, size_t n_blooms, const uint16_t* d_clauses,
                         size_t n_clauses, const uint32_t* d_rule_off, size_t n_rules, const uint32_t* d_query_off,
                         size_t n_queries, uint8_t* d_out, void* stream) {
    if (!c || n_blooms > bb::MAX_BLOOMS || n_queries > bb::MAX_QUERIES ||
        (uint64_t)n_blooms * n_queries > (1ull << 32))
        return GSV_E_INVALID_ARG;
    if (n_queries == 0 || n_blooms == 0) return GSV_SUCCESS;
    if (!filter_args_ok(d_clauses, n_clauses, d_rule_off, n_rules, d_query_off, n_queries) || !d_blooms256 || !d_out)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BLOOM_FILTER, st);
    return hip_err(gsv::launch_bloom_filter(d_blooms256, (uint32_t)n_blooms, d_clauses, (uint32_t)n_clauses, d_rule_off,
                                            (uint32_t)n_rules, d_query_off, (uint32_t)n_queries, d_out, st));
}

int gsv_bloom_filter_batch(gsv_ctx* c, const uint8_t* blooms256, size_t n_blooms, const uint8_t* clause_data,
                           const uint64_t* clause_off, const uint8_t* clause_nil, const uint64_t* rule_off,
                           const uint64_t* query_off, size_t n_queries, uint8_t* out) {
    if (!c || n_blooms > bb::MAX_BLOOMS || n_queries > bb::MAX_QUERIES ||
        (uint64_t)n_blooms * n_queries > (1ull << 32))
        return GSV_E_INVALID_ARG;
    if (n_queries == 0 || n_blooms == 0) return GSV_SUCCESS;
    if (!blooms256 || !out) return GSV_E_INVALID_ARG;
    HostFilter h;
    GSVCHK(host_filter(clause_data, clause_off, clause_nil, rule_off, query_off, n_queries, h));
    Layout L;
    const BloomFilterStage p(L, h.bytes.size(), h.n_clauses(), h.n_rules(), n_queries, n_blooms);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(stage_filter(c, s, p.f, h));
    GSVCHK(s.in(p.blooms, blooms256));
    GSVCHK(gsv_bloom_filter_dev(c, s(p.blooms), n_blooms, s(p.f.idx), h.n_clauses(), s(p.f.rule_off), h.n_rules(),
                                s(p.f.query_off), n_queries, s(p.out), c->stream));
    GSVCHK(s.out(out, p.out));
    return s.finish();
}

}  // extern "C"

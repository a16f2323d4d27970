// The producer side of the C ABI (gsv_ctx.h): the blob codec in both directions (utils.Serialize /
// utils.Deserialize, sharding/utils/marshal.go:71-198) and proposer.createCollation
// (sharding/proposer/proposer.go:55-92) as one prepared call: serialize -> chunk root -> unsigned
// header hash -> crypto.Sign.
#include "blob_codec.h"
#include "gsv_ctx.h"

using namespace gsv::api;
using namespace gsv::blobc;

namespace {

constexpr uint64_t MAX_CHUNKS = 1ull << 31;  // output chunks of one batch (the serialize grid)
constexpr size_t MAX_LISTS = 65535;          // as the notary: k_blob_index / k_blob_strip grid.y

// ---- serialize plan.  Sizes: body i = sum over its blobs of 32 ceil(len / 31); with `limit`, a body
// past 2^20 bytes is marked in `over` and laid out with length 0 (SerializeTxToBlob refuses it).
int ser_sizes(const uint64_t* bo, const uint64_t* lo, size_t n, bool limit, uint64_t* body_off, uint8_t* over) {
    uint64_t pos = 0;
    body_off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if (lo[i + 1] < lo[i]) return GSV_E_INVALID_ARG;
        uint64_t sz = 0;
        for (uint64_t k = lo[i]; k < lo[i + 1]; k++) {
            if (bo[k + 1] < bo[k]) return GSV_E_INVALID_ARG;
            if (bo[k + 1] - bo[k] > 0xFFFFFFFFull) return GSV_E_TOO_LARGE;
            sz += serialized_size(bo[k + 1] - bo[k]);
        }
        const bool ov = limit && !body_fits(sz);
        if (over) over[i] = ov ? 1 : 0;
        if (ov) sz = 0;
        pos += sz;
        if (pos / CHUNK >= MAX_CHUNKS) return GSV_E_TOO_LARGE;
        body_off[i + 1] = pos;
    }
    return GSV_SUCCESS;
}

// key = list offsets, the blob offsets they cover
std::vector<uint64_t> ser_key(const uint64_t* bo, const uint64_t* lo, size_t n) {
    std::vector<uint64_t> k(lo, lo + n + 1);
    if (lo[n] >= lo[0]) k.insert(k.end(), bo + lo[0], bo + lo[n] + 1);
    return k;
}

// the tables of k_blob_serialize: an entry per blob of [lo[0], lo[n]) and the blob of every output chunk
int ser_shape(Shape& s, const uint64_t* bo, const uint64_t* lo, size_t n, bool limit, Layout& L,
              std::vector<uint64_t>& body_off) {
    Shape::BlobSer& sr = s.ser;
    body_off.assign(n + 1, 0);
    std::vector<uint8_t> over(n ? n : 1, 0);
    int rc = ser_sizes(bo, lo, n, limit, body_off.data(), over.data());
    if (rc) return rc;
    const uint64_t k0 = lo[0], nb = lo[n] - lo[0];
    std::vector<BlobEnt> ents(nb ? nb : 1, BlobEnt{0, 0, 0});
    std::vector<uint32_t> cidx(body_off[n] / CHUNK);
    uint64_t chunk = 0;
    for (size_t i = 0; i < n; i++) {
        sr.any_over = sr.any_over || over[i];
        for (uint64_t k = lo[i]; k < lo[i + 1]; k++) {
            const uint32_t len = (uint32_t)(bo[k + 1] - bo[k]);
            ents[k - k0] = BlobEnt{bo[k], len, (uint32_t)chunk};
            if (over[i]) continue;
            const uint64_t nch = num_chunks(len);
            for (uint64_t c = 0; c < nch; c++) cidx[chunk + c] = (uint32_t)(k - k0);
            chunk += nch;
        }
    }
    sr.nchunks = chunk;
    sr.begin = bo[lo[0]];
    sr.end = bo[lo[n]];
    sr.first_blob = k0;
    sr.o_ents = L.add(ents.size() * sizeof(BlobEnt));
    sr.o_cidx = L.add(cidx.size() * 4);
    sr.o_over = L.add(n);
    s.stage(sr.o_ents, ents.data(), ents.size());
    s.stage(sr.o_cidx, cidx.data(), cidx.size());
    s.stage(sr.o_over, over.data(), n);
    return GSV_SUCCESS;
}
int ser_run(const Shape& s, const uint8_t* d_blobs, const uint8_t* d_skip, uint8_t* d_out, hipStream_t st) {
    const Shape::BlobSer& sr = s.ser;
    return hip_err(gsv::launch_blob_serialize(d_blobs, sr.begin, sr.end, s.at<void>(sr.o_ents),
                                              s.at<uint32_t>(sr.o_cidx), d_skip ? d_skip + sr.first_blob : nullptr,
                                              sr.nchunks, d_out, st));
}

// ---- deserialize: key = max_blobs, body offsets
std::vector<uint64_t> deser_key(const uint64_t* h_off, size_t n, uint32_t max_blobs) {
    std::vector<uint64_t> k{max_blobs};
    k.insert(k.end(), h_off, h_off + n + 1);
    return k;
}
uint64_t data_region(uint64_t body_len) { return (CHUNK_DATA * (body_len / CHUNK) + 15) & ~15ull; }
int deser_args(size_t n, uint32_t max_blobs) {
    if (n > MAX_LISTS || max_blobs == 0 || max_blobs > GSV_MAX_TXS_PER_SHARD) return GSV_E_INVALID_ARG;
    return GSV_SUCCESS;
}
int deser_shape(Shape& s, const uint64_t* start, const uint64_t* end, size_t n, uint32_t max_blobs, Layout& L) {
    Shape::BlobDeser& ds = s.deser;
    s.kind = SK_BLOB_DESER;
    std::vector<uint64_t> offs(n), doff(n + 1, 0);
    std::vector<uint32_t> lens(n);
    ds.begin = ~0ull;
    ds.end = 0;
    for (size_t i = 0; i < n; i++) {
        if (end[i] < start[i]) return GSV_E_INVALID_ARG;
        if (end[i] - start[i] > MAX_BODY) return GSV_E_TOO_LARGE;
        offs[i] = start[i];
        lens[i] = (uint32_t)(end[i] - start[i]);
        doff[i + 1] = doff[i] + data_region(lens[i]);
        ds.max_region = std::max(ds.max_region, doff[i + 1] - doff[i]);
        ds.begin = std::min(ds.begin, start[i]);
        ds.end = std::max(ds.end, end[i]);
    }
    ds.o_off = L.add(n * 8);
    ds.o_len = L.add(n * 4);
    ds.o_doff = L.add((n + 1) * 8);
    ds.o_recs = L.add(n * (size_t)max_blobs * sizeof(gsv::BlobRec));
    s.stage(ds.o_off, offs.data(), n);
    s.stage(ds.o_len, lens.data(), n);
    s.stage(ds.o_doff, doff.data(), n + 1);
    return GSV_SUCCESS;
}
// k_blob_index as the notary launches it, its records to arrays, and the indicator bytes stripped
int deser_run(const Shape& s, size_t n, uint32_t max_blobs, const uint8_t* d_bodies, uint32_t* d_nblobs,
              uint32_t* d_start, uint32_t* d_len, uint8_t* d_skip, uint8_t* d_data, hipStream_t st) {
    const Shape::BlobDeser& ds = s.deser;
    HIPCHK(gsv::launch_blob_index(d_bodies, s.at<uint64_t>(ds.o_off), s.at<uint32_t>(ds.o_len), (uint32_t)n, max_blobs,
                                  s.at<void>(ds.o_recs), d_nblobs, st));
    HIPCHK(gsv::launch_blob_unpack(s.at<void>(ds.o_recs), d_nblobs, (uint32_t)n, max_blobs, d_start, d_len, d_skip,
                                   st));
    if (!d_data) return GSV_SUCCESS;
    return hip_err(gsv::launch_blob_strip(d_bodies, ds.begin, ds.end, s.at<uint64_t>(ds.o_off),
                                          s.at<uint32_t>(ds.o_len), s.at<uint64_t>(ds.o_doff), (uint32_t)n,
                                          ds.max_region, d_data, st));
}

// ---- createCollation: the serialize plan with the 2^20 limit + the chunk roots of the bodies it lays out
int proposer_shape(gsv_ctx* c, Shape& s, const uint64_t* bo, const uint64_t* lo, size_t n, Layout& L,
                   std::vector<uint64_t>& body_off) {
    s.kind = SK_PROPOSER;
    int rc = ser_shape(s, bo, lo, n, true, L, body_off);
    if (rc) return rc;
    return chunk_prepare(c, s, s.chunk, L, body_off.data(), body_off.data() + 1, n, MAX_BODY);
}
int proposer_run(gsv_ctx* c, const Shape& s, size_t n, const uint8_t* d_blobs, const uint8_t* d_sid,
                 const uint8_t* d_per, const uint8_t* d_prop, const uint8_t* d_key, uint8_t* d_bodies, uint8_t* d_root,
                 uint8_t* d_hash, uint8_t* d_sig, uint8_t* d_status, hipStream_t st) {
    int rc = ser_run(s, d_blobs, nullptr, d_bodies, st);  // skipEvm false: convertTxToRawBlob
    if (rc) return rc;
    rc = chunk_run(c, s, s.chunk, d_bodies, d_root, st);
    if (rc) return rc;
    {
        KTimer t(c, GSV_K_HEADER, st);
        HIPCHK(gsv::launch_header_hash_unsigned(d_sid, d_root, d_per, d_prop, (uint32_t)n, d_hash, st));
    }
    {
        KTimer t(c, GSV_K_ECRECOVER, st);
        HIPCHK(gsv::launch_ecsign(d_hash, d_key, (uint32_t)n, c->gtab, d_sig, d_status, st));
    }
    if (s.ser.any_over)
        HIPCHK(gsv::launch_proposer_mask(s.at<uint8_t>(s.ser.o_over), (uint32_t)n, d_root, d_hash, d_sig, d_status, st));
    return GSV_SUCCESS;
}

bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// blob offsets rebased so that blob lo[0] starts at 0 (indexable by the caller's blob numbers)
std::vector<uint64_t> rebase(const uint64_t* bo, const uint64_t* lo, size_t n) {
    std::vector<uint64_t> rb(lo[n] + 1, 0);
    for (uint64_t k = lo[0]; k <= lo[n]; k++) rb[k] = bo[k] - bo[lo[0]];
    return rb;
}
int list_args(const uint64_t* bo, const uint64_t* lo, size_t n) {
    if (lo[n] < lo[0]) return GSV_E_INVALID_ARG;
    for (size_t i = 0; i < n; i++)
        if (lo[i + 1] < lo[i]) return GSV_E_INVALID_ARG;
    if (bo[lo[n]] < bo[lo[0]]) return GSV_E_INVALID_ARG;
    return GSV_SUCCESS;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ utils.Serialize
int gsv_blob_serialized_size(const uint64_t* blob_off, const uint64_t* list_off, size_t n_lists,
                             uint64_t* body_off_out) {
    if (!body_off_out || (n_lists && (!blob_off || !list_off))) return GSV_E_INVALID_ARG;
    return ser_sizes(blob_off, list_off, n_lists, false, body_off_out, nullptr);
}

int gsv_blob_serialize_prepare(gsv_ctx* c, const uint64_t* blob_off, const uint64_t* list_off, size_t n_lists) {
    if (!c || (n_lists && (!blob_off || !list_off))) return GSV_E_INVALID_ARG;
    if (n_lists == 0) return GSV_SUCCESS;
    int rc = list_args(blob_off, list_off, n_lists);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    std::vector<uint64_t> body_off;
    return shape_get(c, SK_BLOB_SER, ser_key(blob_off, list_off, n_lists),
                     [&](Shape& ns, Layout& L) {
                         ns.kind = SK_BLOB_SER;
                         return ser_shape(ns, blob_off, list_off, n_lists, false, L, body_off);
                     },
                     &s);
}

int gsv_blob_serialize_batch_dev(gsv_ctx* c, const uint8_t* d_blobs, const uint64_t* blob_off,
                                 const uint8_t* d_skip_evm, const uint64_t* list_off, size_t n_lists,
                                 uint8_t* d_bodies_out, void* stream) {
    if (!c || (n_lists && (!blob_off || !list_off))) return GSV_E_INVALID_ARG;
    if (n_lists == 0) return GSV_SUCCESS;
    int rc = list_args(blob_off, list_off, n_lists);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_BLOB_SER, ser_key(blob_off, list_off, n_lists));
    if (!s) return GSV_E_NOT_PREPARED;
    if (s->ser.nchunks && (!d_blobs || !d_bodies_out || misaligned16(d_bodies_out))) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] { return ser_run(*s, d_blobs, d_skip_evm, d_bodies_out, st); });
}

int gsv_blob_serialize_batch(gsv_ctx* c, const uint8_t* blobs, const uint64_t* blob_off, const uint8_t* skip_evm,
                             const uint64_t* list_off, size_t n_lists, uint8_t* bodies_out, uint64_t* body_off_out) {
    if (!c || !body_off_out || (n_lists && (!blob_off || !list_off))) return GSV_E_INVALID_ARG;
    body_off_out[0] = 0;
    if (n_lists == 0) return GSV_SUCCESS;
    int rc = list_args(blob_off, list_off, n_lists);
    if (rc) return rc;
    rc = ser_sizes(blob_off, list_off, n_lists, false, body_off_out, nullptr);
    if (rc) return rc;
    const uint64_t total = body_off_out[n_lists];
    if (total == 0) return GSV_SUCCESS;
    if (!blobs || !bodies_out) return GSV_E_INVALID_ARG;
    const uint64_t b0 = blob_off[list_off[0]], nbytes = blob_off[list_off[n_lists]] - b0;
    const uint64_t k0 = list_off[0], nblobs = list_off[n_lists] - k0;
    std::vector<uint64_t> rb = rebase(blob_off, list_off, n_lists);
    Layout staged;
    const BlobSerStage p(staged, nbytes, nblobs, skip_evm != nullptr, total);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    std::vector<uint64_t> body_off;
    GSVCHK(shape_temp(c, staged,
                      [&](Shape& ns, Layout& L) {
                          ns.kind = SK_BLOB_SER;
                          return ser_shape(ns, rb.data(), list_off, n_lists, false, L, body_off);
                      },
                      s));
    uint8_t *d_b = sg(p.blobs), *d_sk = sg(p.skip), *d_o = sg(p.bodies);
    GSVCHK(sg.in(p.blobs, blobs + b0));
    if (skip_evm) GSVCHK(sg.in(p.skip, skip_evm + k0));
    // the plan numbers blobs from list_off[0]; the staged flags start there too
    GSVCHK(shape_run(c, s, c->stream, [&] { return ser_run(s, d_b, d_sk ? d_sk - k0 : nullptr, d_o, c->stream); }));
    GSVCHK(sg.out(bodies_out, p.bodies));
    return sg.finish();
}

// ------------------------------------------------------------------ utils.Deserialize
int gsv_blob_data_layout(const uint64_t* off, size_t n, uint64_t* data_off_out) {
    if (!data_off_out || (n && !off)) return GSV_E_INVALID_ARG;
    data_off_out[0] = 0;
    GSVCHK(table_order(off, n, kBlobBodies));
    for (size_t i = 0; i < n; i++) data_off_out[i + 1] = data_off_out[i] + data_region(off[i + 1] - off[i]);
    return GSV_SUCCESS;
}

int gsv_blob_deserialize_prepare(gsv_ctx* c, const uint64_t* h_off, size_t n, uint32_t max_blobs) {
    if (!c || (n && !h_off)) return GSV_E_INVALID_ARG;
    int rc = deser_args(n, max_blobs);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    return shape_get(c, SK_BLOB_DESER, deser_key(h_off, n, max_blobs),
                     [&](Shape& ns, Layout& L) { return deser_shape(ns, h_off, h_off + 1, n, max_blobs, L); }, &s);
}

int gsv_blob_deserialize_batch_dev(gsv_ctx* c, const uint8_t* d_bodies, const uint64_t* h_off, size_t n,
                                   uint32_t max_blobs, uint32_t* d_nblobs, uint32_t* d_blob_start,
                                   uint32_t* d_blob_len, uint8_t* d_skip_evm, uint8_t* d_data, void* stream) {
    if (!c || (n && (!d_bodies || !h_off || !d_nblobs || !d_blob_start || !d_blob_len || !d_skip_evm)) ||
        misaligned16(d_data))
        return GSV_E_INVALID_ARG;
    int rc = deser_args(n, max_blobs);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_BLOB_DESER, deser_key(h_off, n, max_blobs));
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] {
        return deser_run(*s, n, max_blobs, d_bodies, d_nblobs, d_blob_start, d_blob_len, d_skip_evm, d_data, st);
    });
}

int gsv_blob_deserialize_batch(gsv_ctx* c, const uint8_t* bodies, const uint64_t* off, size_t n, uint32_t* nblobs_out,
                               uint64_t* blob_off_out, uint8_t* skip_evm_out, uint8_t* data_out) {
    if (!c || !blob_off_out || (n && (!off || !nblobs_out))) return GSV_E_INVALID_ARG;
    blob_off_out[0] = 0;
    if (n == 0) return GSV_SUCCESS;
    if (n > MAX_LISTS) return GSV_E_INVALID_ARG;
    GSVCHK(table_order(off, n, kBlobBodies));
    uint64_t most = 0;
    for (size_t i = 0; i < n; i++) most = std::max(most, (off[i + 1] - off[i]) / CHUNK);
    if (most == 0) {  // no whole chunk anywhere: no blobs
        for (size_t i = 0; i < n; i++) nblobs_out[i] = 0;
        return GSV_SUCCESS;
    }
    if (!bodies || !skip_evm_out || !data_out) return GSV_E_INVALID_ARG;
    const uint32_t max_blobs = (uint32_t)most;  // every blob takes a chunk: nothing is cut off
    std::vector<uint64_t> st, en, doff(n + 1, 0);
    const uint64_t pos = stage_offsets(off, n, st, en);
    for (size_t i = 0; i < n; i++) doff[i + 1] = doff[i] + data_region(off[i + 1] - off[i]);
    Layout staged;
    const BlobDeserStage p(staged, pos + 16, n, max_blobs, doff[n]);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged,
                      [&](Shape& ns, Layout& L) { return deser_shape(ns, st.data(), en.data(), n, max_blobs, L); }, s));
    uint8_t *d_b = sg(p.bodies), *d_sk = sg(p.skip), *d_d = sg(p.data);
    uint32_t *d_n = sg(p.nblobs), *d_s = sg(p.start), *d_l = sg(p.len);
    GSVCHK(stage_bodies(c, d_b, bodies, off, n, st, en));
    GSVCHK(shape_run(c, s, c->stream,
                     [&] { return deser_run(s, n, max_blobs, d_b, d_n, d_s, d_l, d_sk, d_d, c->stream); }));
    const size_t rows = n * (size_t)max_blobs;
    std::vector<uint32_t> hs(rows), hl(rows);
    std::vector<uint8_t> hk(rows), hd(doff[n]);
    GSVCHK(sg.out(nblobs_out, p.nblobs));
    GSVCHK(sg.out(hs.data(), p.start));
    GSVCHK(sg.out(hl.data(), p.len));
    GSVCHK(sg.out(hk.data(), p.skip));
    GSVCHK(sg.out(hd.data(), p.data));
    GSVCHK(sg.finish());
    // compact into the reference's list of byte strings: the filler between blobs drops out here
    uint64_t k = 0, w = 0;
    for (size_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < nblobs_out[i]; t++) {
            const size_t r = i * (size_t)max_blobs + t;
            memcpy(data_out + w, hd.data() + doff[i] + hs[r], hl[r]);
            skip_evm_out[k] = hk[r];
            w += hl[r];
            blob_off_out[++k] = w;
        }
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ proposer.createCollation
int gsv_proposer_body_layout(const uint64_t* blob_off, const uint64_t* list_off, size_t n, uint64_t* body_off_out,
                             uint8_t* status_out) {
    if (!body_off_out || (n && (!blob_off || !list_off))) return GSV_E_INVALID_ARG;
    std::vector<uint8_t> over(n ? n : 1, 0);
    int rc = ser_sizes(blob_off, list_off, n, true, body_off_out, over.data());
    if (rc) return rc;
    if (status_out)
        for (size_t i = 0; i < n; i++) status_out[i] = over[i] ? GSV_ST_BODY_TOO_LARGE : GSV_ST_OK;
    return GSV_SUCCESS;
}

int gsv_proposer_prepare(gsv_ctx* c, const uint64_t* blob_off, const uint64_t* list_off, size_t n) {
    if (!c || (n && (!blob_off || !list_off)) || n > MAX_LISTS) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = list_args(blob_off, list_off, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    std::vector<uint64_t> body_off;
    return shape_get(c, SK_PROPOSER, ser_key(blob_off, list_off, n),
                     [&](Shape& ns, Layout& L) { return proposer_shape(c, ns, blob_off, list_off, n, L, body_off); },
                     &s);
}

int gsv_proposer_create_collations_dev(gsv_ctx* c, const uint8_t* d_blobs, const uint64_t* blob_off,
                                       const uint64_t* list_off, size_t n, const uint8_t* d_shard_id32,
                                       const uint8_t* d_period32, const uint8_t* d_proposer20,
                                       const uint8_t* d_seckey32, uint8_t* d_bodies_out, uint8_t* d_chunk_root32,
                                       uint8_t* d_hash32, uint8_t* d_sig65, uint8_t* d_status, void* stream) {
    if (!c || n > MAX_LISTS ||
        (n && (!blob_off || !list_off || !d_shard_id32 || !d_period32 || !d_proposer20 || !d_seckey32 ||
               !d_chunk_root32 || !d_hash32 || !d_sig65 || !d_status)))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = list_args(blob_off, list_off, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_PROPOSER, ser_key(blob_off, list_off, n));
    if (!s) return GSV_E_NOT_PREPARED;
    if (s->ser.nchunks && (!d_blobs || !d_bodies_out || misaligned16(d_bodies_out))) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] {
        return proposer_run(c, *s, n, d_blobs, d_shard_id32, d_period32, d_proposer20, d_seckey32, d_bodies_out,
                            d_chunk_root32, d_hash32, d_sig65, d_status, st);
    });
}

int gsv_proposer_create_collations(gsv_ctx* c, const uint8_t* blobs, const uint64_t* blob_off,
                                   const uint64_t* list_off, size_t n, const uint8_t* shard_id32,
                                   const uint8_t* period32, const uint8_t* proposer20, const uint8_t* seckey32,
                                   uint8_t* bodies_out, uint64_t* body_off_out, uint8_t* chunk_root32_out,
                                   uint8_t* hash32_out, uint8_t* sig65_out, uint8_t* status) {
    if (!c || !body_off_out || n > MAX_LISTS ||
        (n && (!blob_off || !list_off || !shard_id32 || !period32 || !proposer20 || !seckey32 || !chunk_root32_out ||
               !hash32_out || !sig65_out || !status)))
        return GSV_E_INVALID_ARG;
    body_off_out[0] = 0;
    if (n == 0) return GSV_SUCCESS;
    int rc = list_args(blob_off, list_off, n);
    if (rc) return rc;
    rc = ser_sizes(blob_off, list_off, n, true, body_off_out, nullptr);
    if (rc) return rc;
    const uint64_t total = body_off_out[n];
    if (total && (!blobs || !bodies_out)) return GSV_E_INVALID_ARG;
    const uint64_t b0 = blob_off[list_off[0]], nbytes = blob_off[list_off[n]] - b0;
    std::vector<uint64_t> rb = rebase(blob_off, list_off, n);
    Layout staged;
    const ProposerStage p(staged, n, nbytes, total);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    std::vector<uint64_t> body_off;
    GSVCHK(shape_temp(c, staged,
                      [&](Shape& ns, Layout& L) { return proposer_shape(c, ns, rb.data(), list_off, n, L, body_off); }, s));
    hipStream_t st = c->stream;
    sg.secret(p.key);  // from here on the keys may be in HBM
    GSVCHK(sg.in(p.key, seckey32));
    if (blobs) GSVCHK(sg.in(p.blobs, blobs + b0));
    GSVCHK(sg.in(p.sid, shard_id32));
    GSVCHK(sg.in(p.per, period32));
    GSVCHK(sg.in(p.prop, proposer20));
    GSVCHK(shape_run(c, s, st, [&] {
        return proposer_run(c, s, n, sg(p.blobs), sg(p.sid), sg(p.per), sg(p.prop), sg(p.key), sg(p.bodies), sg(p.root),
                            sg(p.hash), sg(p.sig), sg(p.st), st);
    }));
    GSVCHK(sg.out(bodies_out, p.bodies));
    GSVCHK(sg.out(chunk_root32_out, p.root));
    GSVCHK(sg.out(hash32_out, p.hash));
    GSVCHK(sg.out(sig65_out, p.sig));
    GSVCHK(sg.out(status, p.st));
    return sg.finish();
}

}  // extern "C"

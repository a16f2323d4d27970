// Merkle-Patricia tries of the C ABI (gsv_ctx.h): chunk roots of collation bodies, DeriveSha over any
// DerivableList, the Proof of Custody, and collation header verification.
#include <map>

#include "gsv_ctx.h"

using namespace gsv::api;

namespace gsv {
namespace api {

// ------------------------------------------------------------------ chunk root launch description
static const uint8_t EMPTY_ROOT[32] = {0x56, 0xe8, 0x1f, 0x17, 0x1b, 0xcc, 0x55, 0xa6, 0xff, 0x83, 0x45,
                                       0xe6, 0x92, 0xc0, 0xf8, 0x6e, 0x5b, 0x48, 0xe0, 0x1b, 0x99, 0x6c,
                                       0xad, 0xc0, 0x01, 0x62, 0x2f, 0xb5, 0xe3, 0x63, 0xb4, 0x21};
static std::vector<Run> runs_of(const std::vector<uint32_t>& idx) {
    std::vector<Run> r;
    size_t k = 0;
    while (k < idx.size()) {
        size_t e = k + 1;
        while (e < idx.size() && idx[e] == idx[e - 1] + 1) e++;
        r.push_back({idx[k], (uint32_t)k, (uint32_t)(e - k)});
        k = e;
    }
    return r;
}

// bodies grouped by length (the trie shape depends only on N, chunk_root.h)
int chunk_prepare(gsv_ctx* c, Shape& s, ChunkLaunch& cl, Layout& L, const uint64_t* start, const uint64_t* end,
                  size_t n, uint64_t max_len) {
    std::map<uint64_t, std::vector<uint32_t>> groups;
    for (size_t i = 0; i < n; i++) {
        if (end[i] < start[i] || end[i] - start[i] > max_len) return GSV_E_TOO_LARGE;
        groups[end[i] - start[i]].push_back((uint32_t)i);
    }
    std::vector<uint64_t> offs;
    offs.reserve(n);
    for (auto& g : groups) {
        if (g.first == 0) {  // empty trie -> emptyRoot (trie/trie.go:472-474)
            cl.empty = g.second;
            continue;
        }
        TrieGroup tg;
        tg.plan = c->plans.get((uint32_t)g.first);
        if (!tg.plan) return GSV_E_NOMEM;
        tg.count = (uint32_t)g.second.size();
        tg.koff = offs.size();
        tg.direct = g.second.size() == n;
        for (uint32_t i : g.second) offs.push_back(start[i]);
        if (!tg.direct) {
            tg.o_roots = L.add((size_t)tg.count * 32);
            tg.runs = runs_of(g.second);
        }
        tg.o_scr = L.add(gsv::chunk_root_scratch_bytes(tg.plan.get(), tg.count));
        cl.groups.push_back(std::move(tg));
    }
    cl.o_off = L.add(offs.size() * 8);
    cl.o_empty = L.add(32);
    s.stage(cl.o_off, offs.data(), offs.size());
    s.stage(cl.o_empty, EMPTY_ROOT, 32);
    return GSV_SUCCESS;
}

int chunk_run(gsv_ctx* c, const Shape& s, const ChunkLaunch& cl, const uint8_t* d_bodies, uint8_t* d_roots,
              hipStream_t st) {
    for (const TrieGroup& g : cl.groups) {
        uint8_t* d_gr = g.direct ? d_roots : s.at<uint8_t>(g.o_roots);
        HIPCHK(gsv::launch_chunk_root_plan(g.plan.get(), d_bodies, s.at<uint64_t>(cl.o_off) + g.koff, g.count,
                                           s.at<uint8_t>(g.o_scr), d_gr, st, hook_begin, hook_end, c));
        for (const Run& r : g.runs)
            HIPCHK(hipMemcpyAsync(d_roots + (size_t)r.dst * 32, d_gr + (size_t)r.from * 32, (size_t)r.count * 32,
                                  hipMemcpyDeviceToDevice, st));
    }
    for (uint32_t i : cl.empty)
        HIPCHK(hipMemcpyAsync(d_roots + (size_t)i * 32, s.at<uint8_t>(cl.o_empty), 32, hipMemcpyDeviceToDevice, st));
    return GSV_SUCCESS;
}

// bodies staged in HBM with 16-byte aligned starts (vector loads in the bottom-level kernel)
uint64_t stage_offsets(const uint64_t* off, size_t n, std::vector<uint64_t>& st, std::vector<uint64_t>& en) {
    st.resize(n);
    en.resize(n);
    uint64_t pos = 0;
    for (size_t i = 0; i < n; i++) {
        st[i] = pos;
        en[i] = pos + (off[i + 1] - off[i]);
        pos = (en[i] + 15) & ~15ull;
    }
    return pos;
}
int stage_bodies(gsv_ctx* c, uint8_t* d_b, const uint8_t* bodies, const uint64_t* off, size_t n,
                 const std::vector<uint64_t>& st, const std::vector<uint64_t>& en) {
    for (size_t i = 0; i < n; i++)
        if (en[i] > st[i])
            HIPCHK(hipMemcpyAsync(d_b + st[i], bodies + off[i], en[i] - st[i], hipMemcpyHostToDevice, c->stream));
    return GSV_SUCCESS;
}

}  // namespace api
}  // namespace gsv

namespace {

constexpr uint64_t MAX_LIST = 1ull << 24;  // generic DeriveSha items per list

// ---- chunk root: key = body offsets
std::vector<uint64_t> chunk_key(const uint64_t* h_off, size_t n) {
    std::vector<uint64_t> k(h_off, h_off + n + 1);
    return k;
}
int chunk_shape(gsv_ctx* c, Shape& s, const uint64_t* start, const uint64_t* end, size_t n, Layout& L) {
    s.kind = SK_CHUNK;
    return chunk_prepare(c, s, s.chunk, L, start, end, n, MAX_BODY);
}

// ---- generic DeriveSha: key = list offsets and the items' value offsets
std::vector<uint64_t> derive_key(const uint64_t* voff, const uint64_t* list_off, size_t n) {
    std::vector<uint64_t> k(list_off, list_off + n + 1);
    k.insert(k.end(), voff + list_off[0], voff + list_off[n] + 1);
    return k;
}
// item k = d_vals[voff[k] .. voff[k+1]); list i = items [list_off[i], list_off[i+1])
int derive_shape(gsv_ctx* c, Shape& s, const uint64_t* voff, const uint64_t* list_off, size_t n, Layout& L) {
    Shape::Derive& dv = s.derive;
    s.kind = SK_DERIVE;
    std::map<uint64_t, std::vector<uint32_t>> groups;
    for (size_t i = 0; i < n; i++) {
        if (list_off[i + 1] < list_off[i]) return GSV_E_INVALID_ARG;
        uint64_t N = list_off[i + 1] - list_off[i];
        if (N > MAX_LIST) return GSV_E_TOO_LARGE;
        groups[N].push_back((uint32_t)i);
    }
    uint64_t total = list_off[n] - list_off[0];
    for (uint64_t k = list_off[0]; k < list_off[n]; k++)
        if (voff[k + 1] < voff[k] || voff[k + 1] - voff[k] >= (1ull << 32)) return GSV_E_INVALID_ARG;
    // per-item leaf message buffers are placed by the kernel (k_derive_leaf): aligned bytes + 32 per item
    uint64_t pos = ((voff[list_off[n]] - voff[list_off[0]] + 7) & ~7ull) + 32ull * total;
    dv.o_voff = L.add((total + 1) * 8);
    dv.o_lmsg = L.add(pos + 256);
    dv.o_leafrefs = L.add(total * 48);
    dv.o_empty = L.add(32);
    s.stage(dv.o_voff, voff + list_off[0], total + 1);
    dv.vend = voff[list_off[n]];
    s.stage(dv.o_empty, EMPTY_ROOT, 32);
    for (auto& g : groups) {
        if (g.first == 0) {  // empty list -> emptyRoot (trie/trie.go:472-474)
            dv.empty = g.second;
            continue;
        }
        TrieGroup tg;
        tg.plan = c->plans.get((uint32_t)g.first, true);
        if (!tg.plan) return GSV_E_NOMEM;
        tg.count = (uint32_t)g.second.size();
        std::vector<uint64_t> base(tg.count);
        for (size_t k = 0; k < tg.count; k++) base[k] = list_off[g.second[k]] - list_off[0];
        tg.o_base = L.add(tg.count * 8);
        tg.o_roots = L.add((size_t)tg.count * 32);
        tg.o_scr = L.add(gsv::derive_sha_scratch_bytes(tg.plan.get(), tg.count));
        tg.runs = runs_of(g.second);
        s.stage(tg.o_base, base.data(), base.size());
        dv.groups.push_back(std::move(tg));
    }
    return GSV_SUCCESS;
}
int derive_run(gsv_ctx* c, const Shape& s, const uint8_t* d_vals, uint8_t* d_roots, hipStream_t st) {
    const Shape::Derive& dv = s.derive;
    for (const TrieGroup& g : dv.groups) {
        uint8_t* d_gr = s.at<uint8_t>(g.o_roots);
        HIPCHK(gsv::launch_derive_sha_plan(g.plan.get(), g.count, d_vals, s.at<uint64_t>(dv.o_voff), dv.vend,
                                           s.at<uint64_t>(g.o_base), s.at<uint8_t>(dv.o_lmsg),
                                           s.at<uint8_t>(dv.o_leafrefs), s.at<uint8_t>(g.o_scr), d_gr, st, hook_begin,
                                           hook_end, c));
        for (const Run& r : g.runs)
            HIPCHK(hipMemcpyAsync(d_roots + (size_t)r.dst * 32, d_gr + (size_t)r.from * 32, (size_t)r.count * 32,
                                  hipMemcpyDeviceToDevice, st));
    }
    for (uint32_t i : dv.empty)
        HIPCHK(hipMemcpyAsync(d_roots + (size_t)i * 32, s.at<uint8_t>(dv.o_empty), 32, hipMemcpyDeviceToDevice, st));
    return GSV_SUCCESS;
}

// ---- Proof of Custody: key = salt, body offsets
std::vector<uint64_t> poc_key(const uint64_t* h_off, size_t n, const uint8_t* salt, size_t slen) {
    std::vector<uint64_t> k;
    key_push_bytes(k, salt, slen);
    k.insert(k.end(), h_off, h_off + n + 1);
    return k;
}
int poc_shape(gsv_ctx* c, Shape& s, const uint64_t* start, const uint64_t* end, size_t n, const uint8_t* salt,
              size_t slen, Layout& L) {
    Shape::Poc& pc = s.poc;
    s.kind = SK_POC;
    std::vector<uint64_t> io(2 * n), oo(n), os(n), oe(n);
    uint64_t pos = 0, mx = 0;
    for (size_t i = 0; i < n; i++) {
        if (end[i] < start[i]) return GSV_E_INVALID_ARG;
        uint64_t len = end[i] - start[i];
        if (len > MAX_POC) return GSV_E_TOO_LARGE;
        uint64_t N = len ? len * (slen + 1) : slen;
        if (N > MAX_POC) return GSV_E_TOO_LARGE;
        io[2 * i] = start[i];
        io[2 * i + 1] = end[i];
        oo[i] = os[i] = pos;
        oe[i] = pos + N;
        mx = N > mx ? N : mx;
        pos = (oe[i] + 15) & ~15ull;
    }
    pc.max = mx;
    pc.salt_len = (uint32_t)slen;
    pc.o_io = L.add(2 * n * 8);
    pc.o_oo = L.add(n * 8);
    pc.o_salt = L.add(slen + 1);
    pc.o_out = L.add(pos + 16);
    s.stage(pc.o_io, io.data(), io.size());
    s.stage(pc.o_oo, oo.data(), oo.size());
    s.stage(pc.o_salt, salt, slen);
    return chunk_prepare(c, s, s.chunk, L, os.data(), oe.data(), n, MAX_POC);
}
int poc_run(gsv_ctx* c, const Shape& s, size_t n, const uint8_t* d_bodies, uint8_t* d_poc, hipStream_t st) {
    const Shape::Poc& pc = s.poc;
    HIPCHK(gsv::launch_poc_expand(d_bodies, s.at<uint64_t>(pc.o_io), s.at<uint64_t>(pc.o_oo), (uint32_t)n, pc.max,
                                  s.at<uint8_t>(pc.o_salt), pc.salt_len, s.at<uint8_t>(pc.o_out), st));
    return chunk_run(c, s, s.chunk, s.at<uint8_t>(pc.o_out), d_poc, st);
}

// ---- collation headers: key = batch size
int header_shape(gsv_ctx*, Shape& s, size_t n, Layout& L) {
    s.kind = SK_HEADER;
    s.header.o_scr = L.add(gsv::header_scratch_bytes((uint32_t)n));
    return GSV_SUCCESS;
}

}  // namespace

namespace gsv {
namespace api {

int derive_prepare(gsv_ctx* c, Shape& s, const uint64_t* voff, const uint64_t* list_off, size_t n, Layout& L) {
    return derive_shape(c, s, voff, list_off, n, L);
}
int derive_launch(gsv_ctx* c, const Shape& s, const uint8_t* d_vals, uint8_t* d_roots, hipStream_t st) {
    return derive_run(c, s, d_vals, d_roots, st);
}

}  // namespace api
}  // namespace gsv

extern "C" {

// ------------------------------------------------------------------ chunk root
int gsv_chunk_root_prepare(gsv_ctx* c, const uint64_t* h_off, size_t n) {
    if (!c || (n && !h_off)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    return shape_get(c, SK_CHUNK, chunk_key(h_off, n),
                     [&](Shape& ns, Layout& L) { return chunk_shape(c, ns, h_off, h_off + 1, n, L); }, &s);
}

int gsv_chunk_root_batch_dev(gsv_ctx* c, const uint8_t* d_bodies, const uint64_t* h_off, size_t n,
                             uint8_t* d_root32_out, void* stream) {
    if (!c || (n && (!h_off || !d_root32_out || !d_bodies))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_CHUNK, chunk_key(h_off, n));
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] { return chunk_run(c, *s, s->chunk, d_bodies, d_root32_out, st); });
}

int gsv_chunk_root_batch(gsv_ctx* c, const uint8_t* bodies, const uint64_t* off, size_t n, uint8_t* root32_out) {
    if (!c || (n && (!off || !root32_out))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(bodies, off, n, kBodies));
    std::vector<uint64_t> st, en;
    uint64_t pos = stage_offsets(off, n, st, en);
    Layout staged;
    const RootsStage p(staged, pos, n);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged, [&](Shape& ns, Layout& L) { return chunk_shape(c, ns, st.data(), en.data(), n, L); },
                      s));
    uint8_t *d_b = sg(p.in), *d_r = sg(p.roots);
    GSVCHK(stage_bodies(c, d_b, bodies, off, n, st, en));
    GSVCHK(shape_run(c, s, c->stream, [&] { return chunk_run(c, s, s.chunk, d_b, d_r, c->stream); }));
    GSVCHK(sg.out(root32_out, p.roots));
    return sg.finish();
}

// ------------------------------------------------------------------ DeriveSha over any DerivableList
static int derive_args(const uint64_t* voff, const uint64_t* list_off, size_t n) {
    return table_order(list_off, n);  // the lists' table; derive_shape checks the values' table it indexes
}

int gsv_derive_sha_prepare(gsv_ctx* c, const uint64_t* voff, const uint64_t* list_off, size_t n) {
    if (!c || (n && (!voff || !list_off))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = derive_args(voff, list_off, n);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    return shape_get(c, SK_DERIVE, derive_key(voff, list_off, n),
                     [&](Shape& ns, Layout& L) { return derive_shape(c, ns, voff, list_off, n, L); }, &s);
}

int gsv_derive_sha_batch_dev(gsv_ctx* c, const uint8_t* d_vals, const uint64_t* voff, const uint64_t* list_off,
                             size_t n, uint8_t* d_root32_out, void* stream) {
    if (!c || (n && (!voff || !list_off || !d_root32_out))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = derive_args(voff, list_off, n);
    if (rc) return rc;
    if (list_off[n] > list_off[0] && !d_vals) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_DERIVE, derive_key(voff, list_off, n));
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] { return derive_run(c, *s, d_vals, d_root32_out, st); });
}

int gsv_derive_sha_batch(gsv_ctx* c, const uint8_t* vals, const uint64_t* voff, const uint64_t* list_off, size_t n,
                         uint8_t* root32_out) {
    if (!c || (n && (!voff || !list_off || !root32_out))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    int rc = derive_args(voff, list_off, n);
    if (rc) return rc;
    uint64_t v0 = voff[list_off[0]], v1 = voff[list_off[n]];
    if (v1 < v0 || (v1 > v0 && !vals)) return GSV_E_INVALID_ARG;
    // stage the values (rebased so item list_off[0] starts at 0)
    std::vector<uint64_t> rv(list_off[n] + 1, 0);
    for (uint64_t k = list_off[0]; k <= list_off[n]; k++) rv[k] = voff[k] - v0;
    Layout staged;
    const RootsStage p(staged, v1 - v0, n);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged, [&](Shape& ns, Layout& L) { return derive_shape(c, ns, rv.data(), list_off, n, L); },
                      s));
    uint8_t *d_v = sg(p.in), *d_r = sg(p.roots);
    GSVCHK(sg.in(p.in, vals + v0, v1 - v0));
    GSVCHK(shape_run(c, s, c->stream, [&] { return derive_run(c, s, d_v, d_r, c->stream); }));
    GSVCHK(sg.out(root32_out, p.roots));
    return sg.finish();
}

// ------------------------------------------------------------------ Proof of Custody
int gsv_collation_poc_prepare(gsv_ctx* c, const uint64_t* h_off, size_t n, const uint8_t* salt, size_t salt_len) {
    if (!c || (n && !h_off) || (salt_len && !salt)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    return shape_get(c, SK_POC, poc_key(h_off, n, salt, salt_len),
                     [&](Shape& ns, Layout& L) { return poc_shape(c, ns, h_off, h_off + 1, n, salt, salt_len, L); },
                     &s);
}

int gsv_collation_poc_batch_dev(gsv_ctx* c, const uint8_t* d_bodies, const uint64_t* h_off, size_t n,
                                const uint8_t* salt, size_t salt_len, uint8_t* d_poc32_out, void* stream) {
    if (!c || (n && (!h_off || !d_poc32_out)) || (salt_len && !salt)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_POC, poc_key(h_off, n, salt, salt_len));
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] { return poc_run(c, *s, n, d_bodies, d_poc32_out, st); });
}

int gsv_collation_poc_batch(gsv_ctx* c, const uint8_t* bodies, const uint64_t* off, size_t n, const uint8_t* salt,
                            size_t salt_len, uint8_t* poc32_out) {
    if (!c || (n && (!off || !poc32_out)) || (salt_len && !salt)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(bodies, off, n, kPocBodies));
    std::vector<uint64_t> st, en;
    uint64_t pos = stage_offsets(off, n, st, en);
    Layout staged;
    const RootsStage p(staged, pos, n);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged,
                      [&](Shape& ns, Layout& L) { return poc_shape(c, ns, st.data(), en.data(), n, salt, salt_len, L); },
                      s));
    uint8_t *d_b = sg(p.in), *d_r = sg(p.roots);
    GSVCHK(stage_bodies(c, d_b, bodies, off, n, st, en));
    GSVCHK(shape_run(c, s, c->stream, [&] { return poc_run(c, s, n, d_b, d_r, c->stream); }));
    GSVCHK(sg.out(poc32_out, p.roots));
    return sg.finish();
}

// ------------------------------------------------------------------ collation header + proposer signature
int gsv_collation_header_prepare(gsv_ctx* c, size_t n) {
    if (!c) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (n > (1u << 30)) return GSV_E_TOO_LARGE;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    return shape_get(c, SK_HEADER, std::vector<uint64_t>{n},
                     [&](Shape& ns, Layout& L) { return header_shape(c, ns, n, L); }, &s);
}

int gsv_collation_header_verify_batch_dev(gsv_ctx* c, const uint8_t* d_sid, const uint8_t* d_root,
                                          const uint8_t* d_per, const uint8_t* d_prop, const uint8_t* d_sig,
                                          const uint8_t* d_nil, size_t n, uint8_t* d_hash, uint8_t* d_signer,
                                          uint8_t* d_st, void* stream) {
    if (!c || (n && (!d_sid || !d_root || !d_per || !d_prop || !d_sig || !d_st))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (n > (1u << 30)) return GSV_E_TOO_LARGE;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_HEADER, std::vector<uint64_t>{n});
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] {
        KTimer t(c, GSV_K_HEADER, st);
        return hip_err(gsv::launch_header_verify(d_sid, d_root, d_per, d_prop, d_sig, d_nil, (uint32_t)n, c->gtab,
                                                 s->at<uint8_t>(s->header.o_scr), d_hash, d_signer, d_st, st));
    });
}

int gsv_collation_header_verify_batch(gsv_ctx* c, const uint8_t* shard_id32, const uint8_t* chunk_root32,
                                      const uint8_t* period32, const uint8_t* proposer20, const uint8_t* sig65,
                                      const uint8_t* nil_flags, size_t n, uint8_t* hash32_out,
                                      uint8_t* signer20_out, uint8_t* status) {
    if (!c || (n && (!shard_id32 || !chunk_root32 || !period32 || !proposer20 || !sig65 || !status)))
        return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (n > (1u << 30)) return GSV_E_TOO_LARGE;
    Layout L;
    const HeaderStage p(L, n, gsv::header_scratch_bytes((uint32_t)n), nil_flags != nullptr, hash32_out != nullptr,
                        signer20_out != nullptr);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.sid, shard_id32));
    GSVCHK(s.in(p.root, chunk_root32));
    GSVCHK(s.in(p.per, period32));
    GSVCHK(s.in(p.prop, proposer20));
    GSVCHK(s.in(p.sig, sig65));
    GSVCHK(s.in(p.nil, nil_flags));
    {
        // s(p.nil), s(p.hash), s(p.signer): nullptr when absent
        KTimer t(c, GSV_K_HEADER, c->stream);
        HIPCHK(gsv::launch_header_verify(s(p.sid), s(p.root), s(p.per), s(p.prop), s(p.sig), s(p.nil), (uint32_t)n,
                                         c->gtab, s(p.scr), s(p.hash), s(p.signer), s(p.st), c->stream));
    }
    GSVCHK(s.out(hash32_out, p.hash));
    GSVCHK(s.out(signer20_out, p.signer));
    GSVCHK(s.out(status, p.st));
    return s.finish();
}

}  // extern "C"

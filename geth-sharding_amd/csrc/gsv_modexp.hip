// The modexp precompile of the C ABI (gsv_ctx.h): header parse and grouping on the host (modexp_plan.h),
// one launch of modexp.hip's kernel per width class.
#include "gsv_ctx.h"
#include "modexp_plan.h"

using namespace gsv::api;
namespace mdx = gsv::mdx;

static_assert(mdx::MAX_LEN == GSV_MODEXP_MAX_LEN, "the cap of gsv.h");

namespace {

// headers, statuses and output offsets of a batch whose table has passed table_check
void layout(const uint8_t* in, const uint64_t* off, size_t n, std::vector<mdx::Header>* hdr, uint64_t* out_off,
            uint8_t* status) {
    out_off[0] = 0;
    for (size_t i = 0; i < n; i++) {
        const mdx::Header h = mdx::parse_header(in + off[i], off[i + 1] - off[i]);
        const bool over = mdx::too_long(h);
        status[i] = over ? GSV_ST_MODEXP_TOO_LONG : GSV_ST_OK;
        out_off[i + 1] = out_off[i] + (over ? 0 : h.mod_len);
        if (hdr) hdr->push_back(h);
    }
}

}  // namespace

extern "C" {

int gsv_modexp_output_layout(const uint8_t* in, const uint64_t* off, size_t n, uint64_t* out_off, uint8_t* status) {
    if (!out_off || (n && (!off || !status))) return GSV_E_INVALID_ARG;
    out_off[0] = 0;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(in, off, n));
    layout(in, off, n, nullptr, out_off, status);
    return GSV_SUCCESS;
}

size_t gsv_modexp_work_bytes(size_t n, uint32_t base_len, uint32_t exp_len, uint32_t mod_len) {
    if (base_len > mdx::MAX_LEN || exp_len > mdx::MAX_LEN) return 0;
    return mdx::work_bytes(n, mod_len);
}

int gsv_modexp_batch_dev(gsv_ctx* c, const uint8_t* d_in, size_t n, uint32_t base_len, uint32_t exp_len,
                         uint32_t mod_len, uint8_t* d_out, uint8_t* d_work, void* stream) {
    if (!c || base_len > mdx::MAX_LEN || exp_len > mdx::MAX_LEN || mod_len > mdx::MAX_LEN || batch_too_long(n))
        return GSV_E_INVALID_ARG;
    if (n == 0 || mod_len == 0) return GSV_SUCCESS;
    if (!d_in || !d_out || (mdx::work_bytes(n, mod_len) && (!d_work || ((uintptr_t)d_work & 3))))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_MODEXP, st);
    return hip_err(gsv::launch_modexp(d_in, (uint32_t)n, base_len, exp_len, mod_len, d_out, d_work, st));
}

int gsv_modexp_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* out,
                     const uint64_t* out_off, uint8_t* status) {
    if (!c || batch_too_long(n) || (n && (!off || !out_off || !status))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    GSVCHK(table_check(in, off, n));
    std::vector<mdx::Header> hdr;
    hdr.reserve(n);
    std::vector<uint64_t> want(n + 1);
    std::vector<uint8_t> st(n);
    layout(in, off, n, &hdr, want.data(), st.data());
    // the caller's table is the layout call's for this input
    if (memcmp(want.data(), out_off, (n + 1) * 8) != 0 || (want[n] && !out)) return GSV_E_INVALID_ARG;
    memcpy(status, st.data(), n);

    std::vector<uint32_t> group[mdx::NCLASS];
    for (size_t i = 0; i < n; i++)
        if (mdx::has_work(hdr[i])) group[mdx::width_class((uint32_t)hdr[i].mod_len)].push_back((uint32_t)i);

    std::unique_lock<std::mutex> lk(c->mu);
    std::vector<uint8_t> rows, res;
    for (int k = 0; k < mdx::NCLASS; k++) {
        const std::vector<uint32_t>& items = group[k];
        const size_t m = items.size();
        if (m == 0) continue;
        uint32_t bw = 0, ew = 0, mw = 0;
        for (uint32_t i : items) {
            bw = std::max(bw, (uint32_t)hdr[i].base_len);
            ew = std::max(ew, (uint32_t)hdr[i].exp_len);
            mw = std::max(mw, (uint32_t)hdr[i].mod_len);
        }
        const size_t row = (size_t)bw + ew + mw;
        rows.resize(m * row);
        res.resize(m * mw);
        for (size_t j = 0; j < m; j++) {
            const uint32_t i = items[j];
            mdx::stage_row(rows.data() + j * row, bw, ew, mw, in + off[i], off[i + 1] - off[i], hdr[i]);
        }
        Layout L;
        const ModexpStage p(L, m * row, m * mw, mdx::work_bytes(m, mw));
        Staged s(c, L, lk);
        if (s.rc) return s.rc;
        GSVCHK(s.in(p.in, rows.data()));
        GSVCHK(gsv_modexp_batch_dev(c, s(p.in), m, bw, ew, mw, s(p.out), s(p.work), c->stream));
        GSVCHK(s.out(res.data(), p.out));
        GSVCHK(s.finish());
        for (size_t j = 0; j < m; j++) {  // the right-aligned modLen bytes of the row
            const uint32_t i = items[j];
            const size_t len = (size_t)hdr[i].mod_len;
            memcpy(out + out_off[i], res.data() + j * mw + (mw - len), len);
        }
    }
    return GSV_SUCCESS;
}

}  // extern "C"

// Logs blooms and receipts of the C ABI (gsv_ctx.h): the device forms check their arguments and enqueue launches
// of receipt.hip; the host form stages a batch of receipt lists, runs scan + bloom + lists, the receipt roots by
// the DeriveSha host plan (gsv_trie.hip) over the same staged bytes, and the compare against the header's values.
#include "gsv_ctx.h"
#include "receipt_host.h"

using namespace gsv::api;
namespace rc = gsv::rc;

namespace {

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int gsv_bloom9_batch_dev(gsv_ctx* c, const uint8_t* d_data, const uint64_t* d_off, size_t n, uint16_t* d_idx_out,
                         void* stream) {
    if (!c || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!d_off || !aligned(d_off, 8) || !d_idx_out || !aligned(d_idx_out, 2)) return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_BLOOM9, st);
    return hip_err(gsv::launch_bloom9(d_data, d_off, (uint32_t)n, d_idx_out, st));
}

int gsv_bloom9_batch(gsv_ctx* c, const uint8_t* data, const uint64_t* off, size_t n, uint16_t* idx_out) {
    if (!c || batch_too_long(n)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (!off || !idx_out) return GSV_E_INVALID_ARG;
    GSVCHK(table_check(data, off, n));
    const size_t bytes = off[n] - off[0];
    const std::vector<uint64_t> rel = table_rebase(off, n);
    Layout L;
    const Bloom9Stage p(L, bytes, n);
    Staged s(c, L);
    if (s.rc) return s.rc;
    GSVCHK(s.in(p.data, data + off[0], bytes));
    GSVCHK(s.in(p.off, rel.data()));
    GSVCHK(gsv_bloom9_batch_dev(c, s(p.data), s(p.off), n, s(p.idx), c->stream));
    GSVCHK(s.out(idx_out, p.idx));
    return s.finish();
}

size_t gsv_receipts_work_bytes(size_t n_receipts, uint64_t vals_bytes) { return rc::work_bytes(n_receipts, vals_bytes); }

int gsv_receipts_bloom_dev(gsv_ctx* c, const uint8_t* d_vals, const uint64_t* d_voff, size_t n, const uint64_t* d_list_off,
                           size_t n_lists, uint64_t vals_bytes, uint8_t* d_work, uint8_t* d_receipt_status,
                           uint8_t* d_receipt_bloom256, uint8_t* d_list_bloom256, uint64_t* d_gas_used,
                           uint8_t* d_list_status, void* stream) {
    if (!c || n > rc::MAX_RECEIPTS || n_lists > rc::MAX_RECEIPTS || vals_bytes > rc::MAX_VALS_BYTES)
        return GSV_E_INVALID_ARG;
    if (n_lists == 0) return GSV_SUCCESS;
    if (!d_list_off || !aligned(d_list_off, 8) || !d_list_bloom256 || !d_gas_used || !aligned(d_gas_used, 8) ||
        !d_list_status)
        return GSV_E_INVALID_ARG;
    if (n && (!d_vals || !d_voff || !aligned(d_voff, 8) || !d_work || !aligned(d_work, 8) || !d_receipt_status))
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    HIPCHK(hipMemsetAsync(d_list_bloom256, 0, n_lists * 256, st));
    if (n) {
        HIPCHK(hipMemsetAsync(d_work, 0, rc::work_offsets(n, vals_bytes).gas, st));  // the descriptor table
        if (d_receipt_bloom256) HIPCHK(hipMemsetAsync(d_receipt_bloom256, 0, n * 256, st));
        {
            KTimer t(c, GSV_K_RECEIPT_SCAN, st);
            HIPCHK(gsv::launch_receipt_scan(d_vals, d_voff, (uint32_t)n, d_list_off, (uint32_t)n_lists, vals_bytes,
                                            d_work, d_receipt_status, st));
        }
        KTimer t(c, GSV_K_RECEIPT_BLOOM, st);
        HIPCHK(gsv::launch_receipt_bloom(d_vals, d_voff, (uint32_t)n, vals_bytes, d_work, d_list_bloom256,
                                         d_receipt_bloom256, st));
    }
    KTimer t(c, GSV_K_RECEIPT_LISTS, st);
    return hip_err(gsv::launch_receipt_lists(d_list_off, (uint32_t)n_lists, (uint32_t)n, vals_bytes, d_work,
                                             d_receipt_status, d_list_bloom256, d_gas_used, d_list_status, st));
}

int gsv_receipts_check_dev(gsv_ctx* c, const uint8_t* d_list_status_in, const uint8_t* d_list_bloom256,
                           uint8_t* d_root32, const uint64_t* d_gas_used, const uint8_t* d_want_bloom256,
                           const uint8_t* d_want_root32, const uint64_t* d_want_gas_used, size_t n_lists,
                           uint8_t* d_status, void* stream) {
    if (!c || n_lists > rc::MAX_RECEIPTS) return GSV_E_INVALID_ARG;
    if (n_lists == 0) return GSV_SUCCESS;
    if (!d_list_status_in || !d_list_bloom256 || !d_root32 || !d_gas_used || !aligned(d_gas_used, 8) ||
        !aligned(d_want_gas_used, 8) || !d_status)
        return GSV_E_INVALID_ARG;
    hipStream_t st = stream_of(c, stream);
    KTimer t(c, GSV_K_RECEIPT_CHECK, st);
    return hip_err(gsv::launch_receipt_check(d_list_status_in, (uint32_t)n_lists, d_list_bloom256, d_root32, d_gas_used,
                                             d_want_bloom256, d_want_root32, d_want_gas_used, d_status, st));
}

int gsv_receipts_verify_batch(gsv_ctx* c, const uint8_t* vals, const uint64_t* voff, const uint64_t* list_off,
                              size_t n_lists, const uint8_t* want_bloom256, const uint8_t* want_root32,
                              const uint64_t* want_gas_used, uint8_t* receipt_status, uint8_t* list_bloom256,
                              uint8_t* root32, uint64_t* gas_used, uint8_t* status) {
    if (!c || n_lists > rc::MAX_RECEIPTS) return GSV_E_INVALID_ARG;
    if (n_lists == 0) return GSV_SUCCESS;
    if (!voff || !list_off || !status) return GSV_E_INVALID_ARG;
    GSVCHK(table_order(list_off, n_lists));
    const size_t n = list_off[n_lists] - list_off[0];
    if (n > rc::MAX_RECEIPTS) return GSV_E_INVALID_ARG;
    const uint64_t* v = voff + list_off[0];
    GSVCHK(table_check(vals, v, n, kBelow4G));
    const uint64_t bytes = v[n] - v[0];
    if (bytes > rc::MAX_VALS_BYTES) return GSV_E_TOO_LARGE;
    // both tables rebased: receipt 0 is the first list's first, and it starts at byte 0 of the staged copy
    const std::vector<uint64_t> rv = table_rebase(v, n), rl = table_rebase(list_off, n_lists);
    Layout staged;
    const ReceiptStage p(staged, bytes, n, n_lists, rc::work_bytes(n, bytes), want_bloom256 != nullptr,
                         want_root32 != nullptr, want_gas_used != nullptr);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged,
                      [&](Shape& ns, Layout& L) { return derive_prepare(c, ns, rv.data(), rl.data(), n_lists, L); }, s));
    GSVCHK(sg.in(p.vals, vals + v[0], bytes));
    GSVCHK(sg.in(p.voff, rv.data()));
    GSVCHK(sg.in(p.loff, rl.data()));
    GSVCHK(sg.in(p.want_bloom, want_bloom256));
    GSVCHK(sg.in(p.want_root, want_root32));
    GSVCHK(sg.in(p.want_gas, want_gas_used));
    GSVCHK(gsv_receipts_bloom_dev(c, sg(p.vals), sg(p.voff), n, sg(p.loff), n_lists, bytes, sg(p.work), sg(p.rstatus),
                                  nullptr, sg(p.lbloom), sg(p.gas), sg(p.lstatus), c->stream));
    uint8_t *d_v = sg(p.vals), *d_r = sg(p.roots);
    GSVCHK(shape_run(c, s, c->stream, [&] { return derive_launch(c, s, d_v, d_r, c->stream); }));
    GSVCHK(gsv_receipts_check_dev(c, sg(p.lstatus), sg(p.lbloom), sg(p.roots), sg(p.gas), sg(p.want_bloom),
                                  sg(p.want_root), sg(p.want_gas), n_lists, sg(p.status), c->stream));
    if (receipt_status) GSVCHK(sg.out(receipt_status, p.rstatus));
    if (list_bloom256) GSVCHK(sg.out(list_bloom256, p.lbloom));
    if (root32) GSVCHK(sg.out(root32, p.roots));
    if (gas_used) GSVCHK(sg.out(gas_used, p.gas));
    GSVCHK(sg.out(status, p.status));
    return sg.finish();
}

}  // extern "C"

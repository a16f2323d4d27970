// BN254 pairing check of the C ABI (gsv_ctx.h): the choice of the launch layout per batch, the prepared
// shape's lane tables, and the bn256Pairing entry points.
#include "gsv_ctx.h"

using namespace gsv::api;

// ---- BN254 pairing: check c = in[off[c] .. off[c+1]); a length that is not a multiple of 192 is
// errBadPairingInput (core/vm/contracts.go:336-338) and contributes no pairs.
// Final exponentiation layout: one lane per check is a ~10^4-product dependent chain; when the batch
// gives the SIMDs fewer than one such wave each, three lanes per check share its exponentiations by
// u (a third of the chain).  GSV_BN_FINAL3 = 0/1 forces the choice (A/B timing).
// From BN_DEEP batches in flight the other batches fill what one small batch leaves idle even at k = 4
// pairs per Miller lane and one lane per check in the final exponentiation (the layout with the fewest
// products): 8,192 checks 3.13 ms per batch at depth 6 against 3.30 for the depth-3 rule's k = 2 /
// three-lane final at depth 4 (r06, profiles/r06/ab/pairing_rank_depth.txt; k = 4 at depth 4: 3.86).
constexpr int BN_DEEP = 6;
// the depth classes whose pairing layouts differ: 1-2, 3-5 (bn_pairs_per_lane's sixth-of-a-wave
// target, no two-lane Miller), 6 and up
int gsv::api::bn_depth_class(int depth) { return depth >= BN_DEEP ? 2 : depth >= 3 ? 1 : 0; }

namespace {

bool bn_final3(size_t nchecks, int cus, int depth) {
    if (const char* e = getenv("GSV_BN_FINAL3")) return atoi(e) != 0;
    return depth < BN_DEEP && nchecks < (size_t)std::max(cus, 1) * 4 * 64;
}
// Two lanes per Miller lane while twice the Miller lanes still fit one wave per SIMD (the Miller
// kernel's register budget admits one wave per SIMD).  GSV_BN_MILLER2 = 0/1 forces the choice.
// With three or more batches in flight (pipeline depth) the other batches' kernels fill the SIMDs a
// small batch leaves idle, so the work-efficient layout wins: no second Miller lane.
bool bn_miller2(size_t nlanes, int cus, int depth) {
    if (const char* e = getenv("GSV_BN_MILLER2")) return atoi(e) != 0;
    return depth < 3 && 2 * nlanes <= (size_t)std::max(cus, 1) * 4 * 64;
}
// The Miller loop at two waves per SIMD (k_bn_miller_w2: one F_p^6 value per lane in LDS, products one
// output coordinate at a time) or at one (k_bn_miller, the default).  The two-wave kernel measured
// slower at every batch size (r05: 65,536 checks at k = 2 11.2 vs 9.8 ms of Miller, k = 4 17.0 vs
// 8.3 ms; 8,192 checks three deep 4.7 vs 3.75 ms per batch, profiles/r05/ab/miller_w2_sweep_*.txt):
// 19 % more VALU per line product and exposed LDS / line-load latency outweigh the second wave.
// GSV_BN_MILLER_W2 = 1 selects it (A/B and its GPU test).
bool bn_miller_w2() {
    if (const char* e = getenv("GSV_BN_MILLER_W2")) return atoi(e) != 0;
    return false;
}
// The Miller loop at two waves per SIMD with each line in LDS (k_bn_miller_l, r05; GSV_BN_MILLER_L = 1).
bool bn_miller_l() {
    if (const char* e = getenv("GSV_BN_MILLER_L")) return atoi(e) != 0;
    return false;
}
// The lines at two waves per SIMD (k_bn_lines_w2: P and Q in LDS, coefficients stored as computed; 256
// registers, no scratch) or at one (k_bn_lines, 256 + 125).  Measured (r05, profiles/r05/ab/lines_w2_*,
// pipe_l*): alone at 65,536 checks 5.95 vs 6.67 ms; in the two-deep pipeline equal (19.98 vs 19.96 ms per
// batch), three deep 19.9-20.0 vs 20.2 ms; at 8,192 checks three deep 4.12 vs 3.75 ms per batch (slower:
// its 512 waves then share SIMDs with the other batches' one-wave Miller / final waves, which a two-wave
// budget cannot join).  So the two-wave kernel is taken from four waves' worth of pairs per SIMD up.
// GSV_BN_LINES_W2 = 0/1 forces the choice.
bool bn_lines_w2(size_t npairs, int cus) {
    if (const char* e = getenv("GSV_BN_LINES_W2")) return atoi(e) != 0;
    return npairs >= (size_t)std::max(cus, 1) * 4 * 64 * 4;
}
// Pairs per Miller lane.  Every lane of a check runs the 64-step loop (its F_p^12 squarings are per
// lane), so k = 4 pairs per lane spends the fewest products; but one lane is a long dependent chain,
// and a batch that gives the GPU's SIMDs fewer than `waves` waves each is latency-bound, so smaller
// batches split a check over more lanes (k = 2, 1).  GSV_BN_PAIRS_PER_LANE forces k (A/B timing).
// At pipeline depth >= 3 a batch only needs a sixth of that (batches overlap): 8,192 checks 4.69 ->
// 3.66 ms per batch at depth 4 with k = 2 and no second Miller lane, 16,384 6.96 -> 6.04 ms at depth 3
// with k = 4 (profiles/r03/ab_pairing_layout_pipe.txt).
uint32_t bn_pairs_per_lane(size_t np, int cus, int depth) {
    if (const char* e = getenv("GSV_BN_PAIRS_PER_LANE")) {
        int k = atoi(e);
        if (k >= 1) return (uint32_t)k;
    }
    if (depth >= BN_DEEP) return 4;  // six or more batches in flight: the most work-efficient layout
    const size_t waves = bn_miller_w2() ? 2 : 1;  // Miller waves per SIMD the kernel's registers admit
    size_t target = (size_t)std::max(cus, 1) * 4 * 64 * waves / (depth >= 3 ? 6 : 1);
    for (uint32_t k = 4; k > 1; k >>= 1)
        if ((np + k - 1) / k >= target) return k;
    return 1;
}
// key: the offsets plus the A/B overrides of the layout choice (tools/pairing_sweep.py)
std::vector<uint64_t> pairing_key(const uint64_t* h_off, size_t n) {
    const char* k = getenv("GSV_BN_PAIRS_PER_LANE");
    const char* f = getenv("GSV_BN_FINAL3");
    const char* m = getenv("GSV_BN_MILLER2");
    const char* cc = getenv("GSV_BN_CONC");
    const char* w2 = getenv("GSV_BN_MILLER_W2");
    const char* lw = getenv("GSV_BN_LINES_W2");
    const char* ml = getenv("GSV_BN_MILLER_L");
    std::vector<uint64_t> key{k ? (uint64_t)atoi(k) + 1 : 0, f ? (uint64_t)atoi(f) + 1 : 0, m ? (uint64_t)atoi(m) + 1 : 0,
                              cc ? (uint64_t)atoi(cc) + 1 : 0, w2 ? (uint64_t)atoi(w2) + 1 : 0, lw ? (uint64_t)atoi(lw) + 1 : 0,
                              ml ? (uint64_t)atoi(ml) + 1 : 0};
    key.insert(key.end(), h_off, h_off + n + 1);
    return key;
}
// depth: batches the caller keeps in flight on this shape (1 for the synchronous host path)
int pairing_shape(gsv_ctx* c, Shape& s, const uint64_t* off, size_t n, Layout& L, int depth) {
    s.kind = SK_PAIRING;
    Shape::Pairing& ps = s.pairing;
    int cus = device_cus(c->device);
    std::vector<uint8_t> bad_len(n, 0);
    size_t np = 0, maxk = 0;
    for (size_t k = 0; k < n; k++) {
        if (off[k + 1] < off[k]) return GSV_E_INVALID_ARG;
        uint64_t len = off[k + 1] - off[k];
        if (len % 192) bad_len[k] = 1;
        else {
            np += len / 192;
            maxk = std::max<size_t>(maxk, len / 192);
        }
    }
    if (np > 0xFFFFFFFFull) return GSV_E_TOO_LARGE;
    // slot-major order: slot k holds the k-th pair of every check that has more than k pairs
    std::vector<uint64_t> per_slot(maxk + 1, 0), slot_base(maxk + 1, 0), fill(maxk + 1, 0);
    for (size_t k = 0; k < n; k++)
        if (!bad_len[k]) per_slot[(off[k + 1] - off[k]) / 192]++;  // histogram of pair counts
    {
        uint64_t more = 0, acc = 0;  // checks with > k pairs, from the top
        std::vector<uint64_t> gt(maxk + 1, 0);
        for (size_t k = maxk + 1; k-- > 0;) {
            gt[k] = more;
            more += per_slot[k];
        }
        for (size_t k = 0; k < maxk; k++) {
            slot_base[k] = acc;
            acc += gt[k];
        }
    }
    std::vector<uint64_t> pair_src(np);
    std::vector<uint32_t> pidx(np), check_first(n + 1);
    size_t q = 0;
    for (size_t k = 0; k < n; k++) {
        check_first[k] = (uint32_t)q;
        if (bad_len[k]) continue;
        size_t slot = 0;
        for (uint64_t o = off[k]; o < off[k + 1]; o += 192, slot++) {
            uint64_t j = slot_base[slot] + fill[slot]++;
            pair_src[j] = o;
            pidx[q++] = (uint32_t)j;
        }
    }
    check_first[n] = (uint32_t)q;
    uint32_t kpl = bn_pairs_per_lane(np, cus, depth);
    std::vector<uint32_t> check_lane(n + 1), lane_first;
    lane_first.reserve(n + np / kpl + 2);
    ps.maxl = 1;
    for (size_t k = 0; k < n; k++) {
        check_lane[k] = (uint32_t)lane_first.size();
        uint32_t b = check_first[k], e = check_first[k + 1];
        lane_first.push_back(b);  // a check without pairs still gets one (empty) lane
        for (uint32_t p = b + kpl; p < e; p += kpl) lane_first.push_back(p);
        ps.maxl = std::max<uint32_t>(ps.maxl, (uint32_t)(lane_first.size() - check_lane[k]));
    }
    check_lane[n] = (uint32_t)lane_first.size();
    lane_first.push_back((uint32_t)q);
    ps.np = np;
    ps.nl = lane_first.size() - 1;
    ps.nchecks = n;
    ps.deep = bn_depth_class(depth);
    ps.layout = (bn_final3(n, cus, depth) ? gsv::GSV_BN_LAYOUT_FINAL3 : 0) |
                (bn_miller2(ps.nl, cus, depth) ? gsv::GSV_BN_LAYOUT_MILLER2 : 0) |
                (bn_miller_w2() ? gsv::GSV_BN_LAYOUT_MILLERW2 : 0) |
                (bn_lines_w2(np, cus) ? gsv::GSV_BN_LAYOUT_LINESW2 : 0) |
                (bn_miller_l() ? gsv::GSV_BN_LAYOUT_MILLERL : 0);
    ps.o_src = L.add(np * 8 + 8);
    ps.o_pidx = L.add(np * 4 + 4);
    ps.o_lfirst = L.add((ps.nl + 1) * 4);
    ps.o_clane = L.add((n + 1) * 4);
    ps.o_cbad = L.add(n);
    ps.o_pstat = L.add(np + 1);
    // the pairs' Miller-loop lines (bn256.hip BN_NLINES).
    // The final exponentiation's workspace (BN_FINAL_SLOTS F_p^12 values per check) reuses the region:
    // the lines are dead once the Miller kernel, which precedes k_bn_final on the run's stream, is done.
    // (a separate region measured the same, r04)
    const size_t lines_bytes = np * 91 * 54 * 4;
    const size_t fws_bytes = n * 108 * 4 * gsv::BN_FINAL_SLOTS;
    ps.o_lines = L.add(std::max(lines_bytes, fws_bytes) + 4);
    ps.o_lstat = L.add(ps.nl + 1);
    ps.o_fv = L.add(ps.nl * 108 * 4 + 4);
    ps.o_fws = ps.o_lines;
    s.stage(ps.o_src, pair_src.data(), np);
    s.stage(ps.o_pidx, pidx.data(), np);
    s.stage(ps.o_lfirst, lane_first.data(), lane_first.size());
    s.stage(ps.o_clane, check_lane.data(), n + 1);
    s.stage(ps.o_cbad, bad_len.data(), n);
    return GSV_SUCCESS;
}
int pairing_run(gsv_ctx* c, const Shape& s, const uint8_t* d_in, uint8_t* d_verdict, hipStream_t st) {
    const Shape::Pairing& ps = s.pairing;
    return hip_err(gsv::launch_bn256_pairing(
        d_in, s.at<uint64_t>(ps.o_src), (uint32_t)ps.np, s.at<uint32_t>(ps.o_lfirst), s.at<uint32_t>(ps.o_pidx),
        (uint32_t)ps.nl, s.at<uint32_t>(ps.o_clane), s.at<uint8_t>(ps.o_cbad), (uint32_t)ps.nchecks,
        s.at<uint8_t>(ps.o_pstat), s.at<uint32_t>(ps.o_lines), s.at<uint8_t>(ps.o_lstat),
        s.at<uint32_t>(ps.o_fv), s.at<uint32_t>(ps.o_fws), ps.maxl, d_verdict, ps.layout, st, hook_begin, hook_end, c));
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ BN254 pairing check
int gsv_bn256_pairing_prepare(gsv_ctx* c, const uint64_t* h_off, size_t n) {
    if (!c || (n && !h_off)) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (batch_too_long(n)) return GSV_E_TOO_LARGE;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    const int depth = std::max(1, c->pipeline_depth);
    int rc = shape_get(c, SK_PAIRING, pairing_key(h_off, n),
                       [&](Shape& ns, Layout& L) { return pairing_shape(c, ns, h_off, n, L, depth); }, &s);
    return rc;
}

int gsv_bn256_pairing_check_batch_dev(gsv_ctx* c, const uint8_t* d_in, const uint64_t* h_off, size_t n,
                                      uint8_t* d_verdict, void* stream) {
    if (!c || (n && (!h_off || !d_verdict))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (batch_too_long(n)) return GSV_E_TOO_LARGE;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_PAIRING, pairing_key(h_off, n));
    if (!s) return GSV_E_NOT_PREPARED;
    if (s->pairing.np && !d_in) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] { return pairing_run(c, *s, d_in, d_verdict, st); });
}

int gsv_bn256_pairing_check_batch(gsv_ctx* c, const uint8_t* in, const uint64_t* off, size_t n, uint8_t* verdict) {
    if (!c || (n && (!off || !verdict))) return GSV_E_INVALID_ARG;
    if (n == 0) return GSV_SUCCESS;
    if (batch_too_long(n)) return GSV_E_TOO_LARGE;
    GSVCHK(table_check(in, off, n));
    const std::vector<uint64_t> rel = table_rebase(off, n);
    Layout staged;
    const PairingStage p(staged, off[n] - off[0], n);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged, [&](Shape& ns, Layout& L) { return pairing_shape(c, ns, rel.data(), n, L, 1); }, s));
    uint8_t *d_in = sg(p.in), *d_v = sg(p.verdict);
    GSVCHK(sg.in(p.in, in + off[0], off[n] - off[0]));
    GSVCHK(shape_run(c, s, c->stream, [&] { return pairing_run(c, s, d_in, d_v, c->stream); }));
    GSVCHK(sg.out(verdict, p.verdict));
    return sg.finish();
}

int gsv_bn256_synth_checks_dev(gsv_ctx* c, uint64_t seed, size_t nchecks, uint8_t* d_out768, uint8_t* d_expect,
                               void* stream) {
    if (!c || (nchecks && !d_out768) || nchecks > 0x3FFFFFFFull) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    return hip_err(gsv::launch_bn256_synth(seed, (uint32_t)nchecks, d_out768, d_expect,
                                           stream_of(c, stream)));
}

}  // extern "C"

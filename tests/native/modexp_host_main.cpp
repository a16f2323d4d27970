// The modexp arithmetic (csrc/modexp_dev.cuh) and the host plan (csrc/modexp_plan.h) as a stand-alone host
// program, built by tests/test_modexp_cpu.py with ASan + UBSan where the compiler links them.
//
//   modexp_host_main FILE
//
// FILE: uint32 count, then per item uint32 input length, uint32 expected length, the input as the
// precompile receives it, the expected output (the model's; empty for an item over the cap).  Every item
// goes through the header parse and the row staging, then through its own width class and the next wider
// one; every fourth item whose exponent has at most 17 bits goes through every wider class as well.  The
// 32-byte class runs in both forms (the unrolled register form and the rolled memory form).  A run in the
// item's own class is made twice, at the item's own lengths and left-padded to wider rows, as the host
// form of the library stages a group; a run in a wider class is made on the padded row.  Every buffer is a heap
// block of exactly the size the code may touch.  Prints "ok"; returns 1 at the first mismatch.
//
//   modexp_host_main --region FILE
//
// The same file format, every item a whole row of the device form.  The numbers are the lane's columns of a
// wave's lane-interleaved region (modexp_item<L, 64, false>, the instantiation the kernel runs, L = 8 added),
// and an item finds its slots as the item before it left them: region_mode below.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../geth-sharding_amd/csrc/modexp_dev.cuh"
#include "../../geth-sharding_amd/csrc/modexp_plan.h"

using namespace gsv::mdx;

template <int L, bool FULL>
static void run_class(const uint8_t* row, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* out) {
    std::unique_ptr<uint32_t[]> s[6];
    for (auto& p : s) p.reset(new uint32_t[L]);
    const Slots w = {s[0].get(), s[1].get(), s[2].get(), s[3].get(), s[4].get(), s[5].get()};
    modexp_item<L, 1, FULL>(row, bl, el, ml, out, w);
}

static void run(int cls, bool full, const uint8_t* row, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* out) {
    switch (cls) {
        case 0: full ? run_class<8, true>(row, bl, el, ml, out) : run_class<8, false>(row, bl, el, ml, out); break;
        case 1: run_class<16, false>(row, bl, el, ml, out); break;
        case 2: run_class<32, false>(row, bl, el, ml, out); break;
        case 3: run_class<64, false>(row, bl, el, ml, out); break;
        case 4: run_class<128, false>(row, bl, el, ml, out); break;
        default: run_class<256, false>(row, bl, el, ml, out); break;
    }
}

// ---------------------------------------------------------------- the lane-interleaved region (--region)
// A wave's region as k_modexp<L> lays it out (csrc/modexp.hip): the numbers are columns of 64 x L words, limb i
// of lane c at word i * 64 + c.  The block is exactly the work_bytes of one wave; where the class keeps the
// products' accumulator in LDS that number is a block of its own of L x 64 words.  The 32-byte class, which
// the kernel runs in registers, gets six columns here as well: the memory form at L = 8.
template <int L>
struct Region {
    static constexpr size_t NUM = (size_t)64 * L;  // words of one number of the wave
    static constexpr uint32_t IN_WORK = L == 8 ? 6 : (L <= LDS_ACC_MAX_LIMBS ? 5 : 6);
    std::unique_ptr<uint32_t[]> work, lds;
    Region() : work(new uint32_t[IN_WORK * NUM]), lds(IN_WORK == 5 ? new uint32_t[NUM] : nullptr) {
        fill(0);
    }
    // kind 0: 0x00, 1: 0xFF, 2: a seeded pattern
    void fill(int kind, uint32_t seed = 1) {
        uint32_t x = seed * 2654435761u + 1u;
        for (uint32_t* p : {work.get(), lds.get()}) {
            if (!p) continue;
            const size_t words = p == work.get() ? IN_WORK * NUM : NUM;
            for (size_t i = 0; i < words; i++) {
                x ^= x << 13, x ^= x >> 17, x ^= x << 5;
                p[i] = kind == 0 ? 0u : kind == 1 ? 0xFFFFFFFFu : x;
            }
        }
    }
    Slots slots(int col) const {
        uint32_t* p = work.get() + col;
        if (IN_WORK == 5) return Slots{p, lds.get() + col, p + NUM, p + 2 * NUM, p + 3 * NUM, p + 4 * NUM};
        return Slots{p, p + NUM, p + 2 * NUM, p + 3 * NUM, p + 4 * NUM, p + 5 * NUM};
    }
    void run(int col, const uint8_t* row, uint32_t bl, uint32_t el, uint32_t ml, uint8_t* out) const {
        modexp_item<L, 64, false>(row, bl, el, ml, out, slots(col));
    }
};

struct Regions {
    Region<8> r8;
    Region<16> r16;
    Region<32> r32;
    Region<64> r64;
    Region<128> r128;
    Region<256> r256;
    template <class F>
    void with(int cls, F f) {
        switch (cls) {
            case 0: f(r8); break;
            case 1: f(r16); break;
            case 2: f(r32); break;
            case 3: f(r64); break;
            case 4: f(r128); break;
            default: f(r256); break;
        }
    }
};

static uint32_t rd32(FILE* f);

// The items of FILE through modexp_item<L, 64, false> in their class's region.  An item's body is its row
// base || exp || mod at the header's lengths, as a launch of the device form gets it.  Each item runs four
// times: in column DIRTY_COL of a region that is never cleared, so on whatever the items of its class before
// it in the file left there; and, in a column that turns with the item, after a fill of the whole region
// with 0x00, with 0xFF and with a seeded pattern.  All four outputs are the expected bytes.
static int region_mode(FILE* f) {
    constexpr int DIRTY_COL = 37;
    std::unique_ptr<Regions> dirty(new Regions), filled(new Regions);
    const uint32_t count = rd32(f);
    size_t runs = 0;
    for (uint32_t it = 0; it < count; it++) {
        const uint32_t ilen = rd32(f), elen = rd32(f);
        std::vector<uint8_t> in(ilen), want(elen);
        if (ilen && fread(in.data(), 1, ilen, f) != ilen) return 2;
        if (elen && fread(want.data(), 1, elen, f) != elen) return 2;
        const Header h = parse_header(in.data(), ilen);
        if (!has_work(h) || ilen != 96 + h.base_len + h.exp_len + h.mod_len || elen != h.mod_len) {
            fprintf(stderr, "item %u: not a whole row of the device form\n", it);
            return 2;
        }
        const uint32_t bl = (uint32_t)h.base_len, el = (uint32_t)h.exp_len, ml = (uint32_t)h.mod_len;
        const int cls = width_class(ml);
        bool sized = false;  // the block is what work_bytes promises a wave
        dirty->with(cls, [&](auto& r) { sized = work_bytes(64, ml) == (cls ? r.IN_WORK * r.NUM * 4 : 0); });
        if (!sized) {
            fprintf(stderr, "item %u: work_bytes is not the region of class %d\n", it, cls);
            return 1;
        }
        // the row in a block of its own size, so that a read past either end is seen
        std::unique_ptr<uint8_t[]> row(new uint8_t[ilen - 96]);
        memcpy(row.get(), in.data() + 96, ilen - 96);
        for (int pass = 0; pass < 4; pass++) {
            std::unique_ptr<uint8_t[]> out(new uint8_t[ml]);
            memset(out.get(), 0xA5, ml);
            if (pass == 0) {
                dirty->with(cls, [&](auto& r) { r.run(DIRTY_COL, row.get(), bl, el, ml, out.get()); });
            } else {
                filled->with(cls, [&](auto& r) {
                    r.fill(pass - 1, it + 1);
                    r.run((int)(it % 64), row.get(), bl, el, ml, out.get());
                });
            }
            runs++;
            if (memcmp(out.get(), want.data(), ml) != 0) {
                fprintf(stderr, "item %u: mismatch in the region of class %d (%s): bl %u el %u ml %u\n", it, cls,
                        pass == 0 ? "slots as the item before left them" : pass == 1 ? "slots of 0x00"
                        : pass == 2 ? "slots of 0xFF" : "slots of a pattern", bl, el, ml);
                return 1;
            }
        }
    }
    fprintf(stderr, "%zu runs\n", runs);
    printf("ok\n");
    return 0;
}

static uint32_t rd32(FILE* f) {
    uint32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "--region") == 0) {
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        const int rc = region_mode(f);
        fclose(f);
        return rc;
    }
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    size_t runs = 0;
    for (uint32_t it = 0; it < count; it++) {
        const uint32_t ilen = rd32(f), elen = rd32(f);
        std::vector<uint8_t> in(ilen), want(elen);
        if (ilen && fread(in.data(), 1, ilen, f) != ilen) return 2;
        if (elen && fread(want.data(), 1, elen, f) != elen) return 2;
        const Header h = parse_header(in.data(), ilen);
        if (!has_work(h)) {
            if (elen != 0) {
                fprintf(stderr, "item %u: no work, but %u bytes expected\n", it, elen);
                return 1;
            }
            continue;
        }
        if (elen != h.mod_len) {
            fprintf(stderr, "item %u: output length %u, header says %llu\n", it, elen, (unsigned long long)h.mod_len);
            return 1;
        }
        const int c0 = width_class((uint32_t)h.mod_len);
        if (work_bytes(1, (uint32_t)h.mod_len) != (c0 ? 64u * work_slots(class_limbs(c0)) * class_limbs(c0) * 4 : 0)) return 1;
        // the exponent's bits, from the staged operand
        std::vector<uint8_t> e(h.exp_len + 1);
        stage_operand(e.data(), h.exp_len, in.data() + (ilen > 96 ? 96 : 0), ilen > 96 ? ilen - 96 : 0, h.base_len,
                      h.exp_len);
        const uint32_t ebits = exp_bits(e.data(), (uint32_t)h.exp_len);
        for (int cls = c0; cls < NCLASS; cls++) {
            if (cls > c0 + 1 && (ebits > 17 || it % 4)) break;
            for (int pad = cls > c0 ? 1 : 0; pad < 2; pad++) {
                // pad: the widths of a group whose longest operands are longer than this item's
                uint32_t bw = (uint32_t)h.base_len, ew = (uint32_t)h.exp_len, mw = (uint32_t)h.mod_len;
                if (pad) {
                    bw = bw + 1 > MAX_LEN ? bw : bw + 1;
                    ew = ew + 2 > MAX_LEN ? ew : ew + 2;
                    mw = 4 * class_limbs(cls);
                }
                const size_t rowlen = (size_t)bw + ew + mw;
                std::unique_ptr<uint8_t[]> row(new uint8_t[rowlen ? rowlen : 1]);
                stage_row(row.get(), bw, ew, mw, in.data(), ilen, h);
                for (int full = 0; full < (cls == 0 ? 2 : 1); full++) {
                    std::unique_ptr<uint8_t[]> out(new uint8_t[mw]);
                    memset(out.get(), 0xA5, mw);
                    run(cls, full != 0, row.get(), bw, ew, mw, out.get());
                    runs++;
                    bool ok = memcmp(out.get() + (mw - elen), want.data(), elen) == 0;
                    for (uint32_t i = 0; i < mw - elen; i++) ok = ok && out[i] == 0;
                    if (!ok) {
                        fprintf(stderr, "item %u: mismatch in class %d (form %d, padded %d): bl %u el %u ml %u\n", it,
                                cls, full, pad, bw, ew, mw);
                        return 1;
                    }
                }
            }
        }
    }
    fclose(f);
    fprintf(stderr, "%zu runs\n", runs);
    printf("ok\n");
    return 0;
}

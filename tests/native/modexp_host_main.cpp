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

static uint32_t rd32(FILE* f) {
    uint32_t v = 0;
    if (fread(&v, 4, 1, f) != 1) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

int main(int argc, char** argv) {
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

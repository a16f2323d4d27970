// Stand-alone CPU run of csrc/blob_codec.h, the text the kernels of csrc/blob.hip run on the GPU
// (tests/test_blob_codec_host.py builds it with g++, with ASan + UBSan when the compiler links them, and
// runs it as a child process).
//
//   blob_codec_host IN OUT
//
// IN (little-endian): u32 cases, then per case
//   u32 kind = 0 (serialize): u32 align, u32 n_lists, u64 list_off[n_lists + 1], u32 nblobs,
//                             u64 blob_off[nblobs + 1], u8 skip_evm[nblobs], blob bytes
//       OUT: u64 body_off[n_lists + 1], the bodies: serialize_group over every 16-byte group, through the
//            same plan tables (an entry per blob, a blob index per output chunk) the kernel reads
//   u32 kind = 1 (deserialize): u32 align, u64 len, body bytes
//       OUT: u32 nblobs, then per blob u32 len, u8 skip_evm, its bytes: index_body, and strip_word over
//            every word of the data region
// The source bytes of a case are copied to the END of a heap block of their own at `align` (0..3) bytes
// past a 4-byte boundary, 0xFF before them, so that a load past the end runs into the allocator's
// red zone and a load before the start reads 0xFF.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../geth-sharding_amd/csrc/blob_codec.h"

using namespace gsv::blobc;

static FILE *fin, *fout;

template <typename T>
static T rd() {
    T v;
    if (fread(&v, sizeof(T), 1, fin) != 1) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return v;
}
static void rdn(void* p, size_t n) {
    if (n && fread(p, 1, n, fin) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}
static void wr(const void* p, size_t n) {
    if (n && fwrite(p, 1, n, fout) != n) exit(3);
}

// `n` bytes from the input at base + 4 + align, ending where the block ends
struct Placed {
    uint8_t* block;
    uint8_t* p;
    Placed(size_t n, uint32_t align) {
        block = (uint8_t*)malloc(4 + align + n);
        memset(block, 0xFF, 4 + align);
        p = block + 4 + align;
        rdn(p, n);
    }
    ~Placed() { free(block); }
};

static void do_serialize() {
    const uint32_t align = rd<uint32_t>(), n = rd<uint32_t>();
    std::vector<uint64_t> lo(n + 1);
    rdn(lo.data(), 8 * (n + 1));
    const uint32_t nb = rd<uint32_t>();
    std::vector<uint64_t> bo(nb + 1);
    rdn(bo.data(), 8 * (nb + 1));
    std::vector<uint8_t> skip(nb + 1);
    rdn(skip.data(), nb);
    Placed src(bo[nb], align);
    // the plan, as ser_shape (csrc/gsv_proposer.hip) builds it
    std::vector<uint64_t> body_off(n + 1, 0);
    std::vector<BlobEnt> ents(nb + 1);
    std::vector<uint32_t> cidx;
    for (uint32_t i = 0; i < n; i++) {
        for (uint64_t k = lo[i]; k < lo[i + 1]; k++) {
            const uint32_t len = (uint32_t)(bo[k + 1] - bo[k]);
            ents[k] = BlobEnt{bo[k], len, (uint32_t)cidx.size()};
            for (uint64_t c = 0; c < num_chunks(len); c++) cidx.push_back((uint32_t)k);
        }
        body_off[i + 1] = (uint64_t)CHUNK * cidx.size();
    }
    std::vector<uint32_t> out(8 * cidx.size() + 4);
    const Src s = make_src(src.p, n ? bo[lo[0]] : 0, n ? bo[lo[n]] : 0);
    for (uint64_t g = 0; g < 2 * cidx.size(); g++) {  // the kernel's lane g
        const uint32_t cg = (uint32_t)(g >> 1), h = (uint32_t)(g & 1);
        const BlobEnt e = ents[cidx[cg]];
        const uint32_t c = cg - e.first;
        uint32_t f = 0;
        if (h == 0 && c + 1 == (uint32_t)num_chunks(e.len)) f = skip[cidx[cg]];
        serialize_group(s, e.off, e.len, f, c, h, &out[4 * g]);
    }
    wr(body_off.data(), 8 * (n + 1));
    wr(out.data(), body_off[n]);
}

static void do_deserialize() {
    const uint32_t align = rd<uint32_t>();
    const uint64_t len = rd<uint64_t>();
    Placed src(len, align);
    const uint32_t nch = (uint32_t)(len / CHUNK);
    std::vector<BlobSpan> spans(nch + 1);
    const uint32_t nblobs = index_body(src.p, len, spans.data(), nch);
    const uint32_t words = (CHUNK_DATA * nch + 3) / 4;
    std::vector<uint32_t> data(words + 1);
    const Src s = make_src(src.p, 0, len);
    for (uint32_t w = 0; w < words; w++) data[w] = strip_word(s, 0, nch, w);
    wr(&nblobs, 4);
    for (uint32_t t = 0; t < nblobs; t++) {
        const uint8_t sk = (uint8_t)spans[t].skip_evm;
        wr(&spans[t].len, 4);
        wr(&sk, 1);
        wr((const uint8_t*)data.data() + CHUNK_DATA * spans[t].first_chunk, spans[t].len);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    fin = fopen(argv[1], "rb");
    fout = fopen(argv[2], "wb");
    if (!fin || !fout) return 2;
    const uint32_t cases = rd<uint32_t>();
    for (uint32_t i = 0; i < cases; i++) {
        const uint32_t kind = rd<uint32_t>();
        if (kind == 0) do_serialize();
        else do_deserialize();
    }
    fclose(fin);
    fclose(fout);
    printf("ok %u\n", cases);
    return 0;
}

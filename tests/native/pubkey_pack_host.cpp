// Stand-alone check of the host packing of public keys (csrc/pubkey_pack.h) and of the staging plans of
// the two host entry points that use it (csrc/staging.h VerifyStage, PubkeyParseStage).  Every input
// and output buffer is a heap block of exactly the bytes it may touch, so under AddressSanitizer a read
// past the last key or a write past a row faults.  Prints "ok <checks>" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../geth-sharding_amd/csrc/pubkey_pack.h"
#include "../../geth-sharding_amd/csrc/staging.h"

static int g_fail = 0, g_checks = 0;

static void expect(bool ok, const char* what, size_t i) {
    g_checks++;
    if (!ok) {
        printf("FAIL %s (key %zu)\n", what, i);
        g_fail++;
    }
}

// packs keys of the given lengths, laid end to end from `lead` bytes into a buffer that ends with the
// last key, and checks every row and length byte
static void run(const std::vector<size_t>& lens, size_t lead) {
    const size_t n = lens.size();
    size_t total = lead;
    for (size_t l : lens) total += l;
    uint8_t* pub = total ? (uint8_t*)malloc(total) : nullptr;
    for (size_t i = 0; i < total; i++) pub[i] = (uint8_t)(1 + i % 251);  // no zero byte in a key
    uint64_t* off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    off[0] = lead;
    for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + lens[i];
    uint8_t* rows = n ? (uint8_t*)malloc(n * 65) : nullptr;
    uint8_t* len = n ? (uint8_t*)malloc(n) : nullptr;
    if (n) {
        memset(rows, 0xEE, n * 65);
        memset(len, 0xEE, n);
    }
    gsv::pubkey_pack(pub, off, n, rows, len);
    for (size_t i = 0; i < n; i++) {
        const size_t keep = (lens[i] == 33 || lens[i] == 65) ? lens[i] : 0;
        expect(len[i] == keep, "length byte", i);
        expect(keep == 0 || memcmp(rows + i * 65, pub + off[i], keep) == 0, "key bytes", i);
        bool pad = true;
        for (size_t k = keep; k < 65; k++) pad = pad && rows[i * 65 + k] == 0;
        expect(pad, "zero padding", i);
    }
    free(len);
    free(rows);
    free(off);
    free(pub);
}

template <typename S>
static void plan(const S&, const gsv::api::Layout& L, std::vector<gsv::api::B8> bufs, const char* name) {
    size_t sum = 0;
    for (size_t i = 0; i < bufs.size(); i++) {
        expect(bufs[i].off % 256 == 0 && bufs[i].off + bufs[i].bytes <= L.n, name, i);
        expect(bufs[i].off == sum, name, i);  // in arena order, back to back: no two overlap
        sum += gsv::api::al(bufs[i].bytes ? bufs[i].bytes : 1);
    }
    expect(sum == L.n, name, bufs.size());
}

int main() {
    run({}, 0);                                    // an empty batch
    run({}, 7);
    for (size_t l : {(size_t)0, (size_t)1, (size_t)33, (size_t)65, (size_t)66, (size_t)1 << 16}) {
        run({l}, 0);                               // alone: the key ends the buffer
        run({l}, 5);
    }
    run({0, 1, 33, 65, 66, (size_t)1 << 16, 65, 33}, 0);  // together; the last key ends the buffer
    run({65, 0, 0, 33, 32, 34, 64, 66, 65}, 3);
    run({33, 33, 0}, 0);                           // the last key is empty and the buffer ends with it
    for (size_t n : {(size_t)1, (size_t)3, (size_t)257}) {
        {
            gsv::api::Layout L;
            gsv::api::VerifyStage p(L, n);
            expect(p.msg.bytes == n * 32 && p.sig.bytes == n * 64 && p.pub.bytes == n * 65 && p.len.bytes == n &&
                       p.ok.bytes == n,
                   "VerifyStage sizes", n);
            plan(p, L, {p.msg, p.sig, p.pub, p.len, p.ok}, "VerifyStage");
        }
        {
            gsv::api::Layout L;
            gsv::api::PubkeyParseStage p(L, n);
            expect(p.pub.bytes == n * 65 && p.len.bytes == n && p.out.bytes == n * 65 && p.ok.bytes == n,
                   "PubkeyParseStage sizes", n);
            plan(p, L, {p.pub, p.len, p.out, p.ok}, "PubkeyParseStage");
        }
    }
    if (g_fail) {
        printf("%d failure(s)\n", g_fail);
        return 1;
    }
    printf("ok %d\n", g_checks);
    return 0;
}

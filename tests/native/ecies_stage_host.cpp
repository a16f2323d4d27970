// Stand-alone check of the staging plans of gsv_ecies_decrypt_batch and gsv_ecies_encrypt_batch
// (csrc/staging.h EciesDecryptStage, EciesEncryptStage), in the manner of ecdh_stage_host.cpp: every
// offset 256-aligned, the buffers pairwise disjoint and of the sizes the entry points copy, the total
// exactly the buffers' rounded sizes, s2 and its table reserving nothing when absent; and what the
// secret rule of the host forms rests on: the secret regions (the keys, the work area with Ke || Km,
// the plaintext) are FIRST and contiguous from offset 0, `secret` is exactly the end of the last one's
// slots, and every buffer that is not secret starts at or behind it.  Prints "ok <plans>", exits 0.
#include <cstdio>
#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/staging.h"

using namespace gsv::api;

struct Region { const char* name; size_t off, bytes, want; bool present, secret; };

static int g_fail = 0, g_plans = 0;
static uint8_t* const kBase = (uint8_t*)(uintptr_t)0x10000;  // never dereferenced

template <typename T>
static Region reg(const char* name, const Buf<T>& b, size_t want, bool secret, bool present = true) {
    if (present != (b(kBase) != nullptr)) {
        printf("FAIL %s: present=%d but pointer %p\n", name, (int)present, (void*)b(kBase));
        g_fail++;
    }
    return {name, b.off, b.bytes, present ? want : 0, present, secret};
}

// rs in arena order
static void check(const std::string& plan, const Layout& L, const std::vector<Region>& rs, size_t secret) {
    g_plans++;
    auto fail = [&](const char* what, const Region& r) {
        printf("FAIL %s: %s (%s off=%zu bytes=%zu secret=%zu total=%zu)\n", plan.c_str(), what, r.name, r.off, r.bytes,
               secret, L.n);
        g_fail++;
    };
    size_t sum = 0, next = 0, secret_end = 0, nsecret = 0;
    bool seen_public = false;
    for (size_t i = 0; i < rs.size(); i++) {
        const Region& a = rs[i];
        if (!a.present) {
            if (a.off != kAbsent || a.bytes != 0) fail("an absent buffer reserves something", a);
            continue;
        }
        if (a.off % 256) fail("offset not 256-aligned", a);
        if (a.bytes != a.want) fail("not the size the entry point copies", a);
        if (a.off + a.bytes > L.n) fail("ends past the total", a);
        if (a.off != next) fail("not contiguous with the region before it", a);
        next = a.off + al(a.bytes ? a.bytes : 1);
        sum += al(a.bytes ? a.bytes : 1);
        for (size_t j = i + 1; j < rs.size(); j++) {
            const Region& b = rs[j];
            if (b.present && a.off < b.off + (b.bytes ? b.bytes : 1) && b.off < a.off + (a.bytes ? a.bytes : 1))
                fail("overlaps another buffer", a);
        }
        if (a.secret) {
            if (seen_public) fail("a secret region behind a public one", a);
            secret_end = next;
            nsecret++;
        } else {
            seen_public = true;
            if (a.off < secret) fail("a public buffer inside the wiped range", a);
        }
    }
    if (sum != L.n) fail("total is not the sum of the buffers", rs[0]);
    if (rs[0].off != 0 || !rs[0].secret) fail("the keys are not the first region", rs[0]);
    if (nsecret != 3) fail("keys, work area and plaintext are not all secret", rs[0]);
    if (secret != secret_end) fail("the wipe length is not the end of the last secret region", rs[0]);
    if (secret == 0 || secret > L.n) fail("the wipe length is outside the stage", rs[0]);
}

int main() {
    const size_t kDec = 113, kEnc = 115;  // gsv_ecies_work_bytes per item
    for (size_t n : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)1 << 20}) {
        for (size_t per : {(size_t)0, (size_t)1, (size_t)307, (size_t)4209}) {  // bytes per item
            for (int s2 = 0; s2 < 3; s2++) {  // no s2 table; a table of empty strings; 2 bytes each
                const bool has = s2 > 0;
                const size_t bytes = n * per, s2b = s2 == 2 ? 2 * n : 0;
                const std::string tag = " n=" + std::to_string(n) + " per=" + std::to_string(per) + " s2=" + std::to_string(s2);
                {
                    Layout L;
                    EciesDecryptStage p(L, n, kDec, bytes, s2b, has);
                    check("ecies_decrypt" + tag, L,
                          {reg("key", p.key, n * 32, true), reg("work", p.work, n * kDec, true),
                           reg("msg", p.msg, bytes, true), reg("ct", p.ct, bytes, false),
                           reg("off", p.off, (n + 1) * 8, false), reg("s2", p.s2, s2b, false, has),
                           reg("s2off", p.s2off, (n + 1) * 8, false, has), reg("mlen", p.mlen, n * 4, false),
                           reg("st", p.st, n, false)},
                          p.secret);
                }
                {
                    Layout L;
                    EciesEncryptStage p(L, n, kEnc, bytes, s2b, has);
                    check("ecies_encrypt" + tag, L,
                          {reg("key", p.key, n * 32, true), reg("work", p.work, n * kEnc, true),
                           reg("msg", p.msg, bytes, true), reg("pub", p.pub, n * 64, false), reg("iv", p.iv, n * 16, false),
                           reg("off", p.off, (n + 1) * 8, false), reg("s2", p.s2, s2b, false, has),
                           reg("s2off", p.s2off, (n + 1) * 8, false, has), reg("ct", p.ct, bytes + n * 113, false),
                           reg("st", p.st, n, false)},
                          p.secret);
                }
            }
        }
    }
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("ok %d\n", g_plans);
    return 0;
}

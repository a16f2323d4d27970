// Stand-alone check of the staging plans of gsv_ecdsa_sign_batch and gsv_pubkey_create_batch
// (csrc/staging.h SignStage, PubkeyCreateStage), in the manner of staging_host.cpp: every offset
// 256-aligned, the buffers pairwise disjoint and of the sizes the entry points copy, the total exactly
// the buffers' rounded sizes, an absent address buffer reserving nothing; and what the secret-key rule
// of the host forms rests on: the keys are the FIRST region (offset 0, n x 32 bytes), and no other
// buffer starts inside the 256-B slots the wipe's n x 32 bytes fall in.  Prints "ok <plans>", exits 0.
#include <cstdio>
#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/staging.h"

using namespace gsv::api;

struct Region { const char* name; size_t off, bytes, want; bool present; };

static int g_fail = 0, g_plans = 0;
static uint8_t* const kBase = (uint8_t*)(uintptr_t)0x10000;  // never dereferenced

static Region reg(const char* name, const B8& b, size_t want, bool present = true) {
    if (present != (b(kBase) != nullptr)) {
        printf("FAIL %s: present=%d but pointer %p\n", name, (int)present, (void*)b(kBase));
        g_fail++;
    }
    return {name, b.off, b.bytes, want, present};
}

static void check(const std::string& plan, const Layout& L, const std::vector<Region>& rs, size_t n) {
    g_plans++;
    auto fail = [&](const char* what, const Region& r) {
        printf("FAIL %s: %s (%s off=%zu bytes=%zu total=%zu)\n", plan.c_str(), what, r.name, r.off, r.bytes, L.n);
        g_fail++;
    };
    size_t sum = 0;
    for (size_t i = 0; i < rs.size(); i++) {
        const Region& a = rs[i];
        if (!a.present) continue;
        if (a.off % 256) fail("offset not 256-aligned", a);
        if (a.bytes != a.want) fail("not the size the entry point copies", a);
        if (a.off + a.bytes > L.n) fail("ends past the total", a);
        sum += al(a.bytes ? a.bytes : 1);
        for (size_t j = i + 1; j < rs.size(); j++) {
            const Region& b = rs[j];
            if (b.present && a.off < b.off + (b.bytes ? b.bytes : 1) && b.off < a.off + (a.bytes ? a.bytes : 1))
                fail("overlaps another buffer", a);
        }
    }
    if (sum != L.n) fail("total is not the sum of the buffers", rs[0]);
    // the keys come first, and the wipe of [0, 32 n) touches no other buffer
    if (rs[0].off != 0 || rs[0].bytes != n * 32) fail("the keys are not the first region", rs[0]);
    for (size_t i = 1; i < rs.size(); i++)
        if (rs[i].present && rs[i].off < al(n * 32)) fail("starts inside the keys' slots", rs[i]);
}

int main() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)8, (size_t)9, (size_t)4096}) {
        const std::string tag = " n=" + std::to_string(n);
        {
            Layout L;
            SignStage p(L, n);
            check("ecdsa_sign_batch" + tag, L,
                  {reg("key", p.key, n * 32), reg("msg", p.msg, n * 32), reg("sig", p.sig, n * 65), reg("st", p.st, n)},
                  n);
        }
        for (bool opt : {false, true}) {
            Layout L;
            PubkeyCreateStage p(L, n, opt);
            check("pubkey_create_batch" + tag + (opt ? " +addr" : " -addr"), L,
                  {reg("key", p.key, n * 32), reg("pub", p.pub, n * 65), reg("addr", p.addr, opt ? n * 20 : 0, opt),
                   reg("st", p.st, n)},
                  n);
        }
    }
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("ok %d\n", g_plans);
    return 0;
}

// Stand-alone check of the staging plans of gsv_proposer_create_collations, gsv_blob_serialize_batch and
// gsv_blob_deserialize_batch (csrc/staging.h ProposerStage, BlobSerStage, BlobDeserStage), in the manner of
// sign_stage_host.cpp: every offset 256-aligned, the buffers pairwise disjoint and of the sizes the entry
// points copy, the total exactly the buffers' rounded sizes, an absent flag buffer reserving nothing; and
// what the proposer's secret-key rule rests on: the keys are the FIRST region (offset 0, n x 32 bytes), and
// no other buffer starts inside the 256-B slots the wipe's n x 32 bytes fall in.  Prints "ok <plans>".
#include <cstdio>
#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/staging.h"

using namespace gsv::api;

struct Region { const char* name; size_t off, bytes, want; bool present; };

static int g_fail = 0, g_plans = 0;
static uint8_t* const kBase = (uint8_t*)(uintptr_t)0x10000;  // never dereferenced

template <typename T>
static Region reg(const char* name, const Buf<T>& b, size_t want, bool present = true) {
    if (present != (b(kBase) != nullptr)) {
        printf("FAIL %s: present=%d but pointer %p\n", name, (int)present, (void*)b(kBase));
        g_fail++;
    }
    return {name, b.off, b.bytes, want, present};
}

static void check(const std::string& plan, const Layout& L, const std::vector<Region>& rs, size_t keys) {
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
    if (!keys) return;
    // the keys come first, and the wipe of [0, 32 n) touches no other buffer
    if (rs[0].off != 0 || rs[0].bytes != keys * 32) fail("the keys are not the first region", rs[0]);
    for (size_t i = 1; i < rs.size(); i++)
        if (rs[i].present && rs[i].off < al(keys * 32)) fail("starts inside the keys' slots", rs[i]);
}

int main() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)8, (size_t)9, (size_t)4096}) {
        const std::string tag = " n=" + std::to_string(n);
        for (size_t blob_bytes : {(size_t)0, (size_t)1, (size_t)100000}) {
            const size_t body_bytes = 32 * ((blob_bytes + 30) / 31);
            {
                Layout L;
                ProposerStage p(L, n, blob_bytes, body_bytes);
                check("proposer_create_collations" + tag, L,
                      {reg("key", p.key, n * 32), reg("blobs", p.blobs, blob_bytes), reg("sid", p.sid, n * 32),
                       reg("per", p.per, n * 32), reg("prop", p.prop, n * 20), reg("bodies", p.bodies, body_bytes),
                       reg("root", p.root, n * 32), reg("hash", p.hash, n * 32), reg("sig", p.sig, n * 65),
                       reg("st", p.st, n)},
                      n);
            }
            for (bool skip : {false, true}) {
                Layout L;
                BlobSerStage p(L, blob_bytes, n, skip, body_bytes);
                check("blob_serialize_batch" + tag, L,
                      {reg("blobs", p.blobs, blob_bytes), reg("skip", p.skip, skip ? n : 0, skip),
                       reg("bodies", p.bodies, body_bytes)},
                      0);
            }
        }
        for (uint32_t max_blobs : {1u, 5u, 32768u}) {
            Layout L;
            BlobDeserStage p(L, 12345, n, max_blobs, 9984);
            check("blob_deserialize_batch" + tag, L,
                  {reg("bodies", p.bodies, 12345), reg("nblobs", p.nblobs, n * 4),
                   reg("start", p.start, n * max_blobs * 4), reg("len", p.len, n * max_blobs * 4),
                   reg("skip", p.skip, n * max_blobs), reg("data", p.data, 9984)},
                  0);
        }
    }
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("ok %d\n", g_plans);
    return 0;
}

// Stand-alone known-answer run of the host build of csrc/sha256_dev.cuh and csrc/rfc6979_dev.cuh
// (rfc6979_host.cpp's exports), meant to be compiled with ASan + UBSan and run as a child process
// (tests/test_rfc6979_cpu.py): SHA-256 at the padding's edges against FIPS 180-4's and NIST's vectors,
// and RFC 6979 A.2.5's nonce at counter 0 with three further counters drawn.  Prints "ok", exits 0.
#include <cstdio>
#include <cstring>
#include <string>

#include "rfc6979_host.cpp"

static std::string hex(const uint8_t* b, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) {
        s += d[b[i] >> 4];
        s += d[b[i] & 15];
    }
    return s;
}
static void unhex(uint8_t* out, const char* h) {
    for (size_t i = 0; h[2 * i]; i++) {
        unsigned v;
        sscanf(h + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}

int main() {
    int fail = 0;
    auto expect = [&](const std::string& got, const char* want, const char* what) {
        if (got != want) {
            printf("FAIL %s: %s != %s\n", what, got.c_str(), want);
            fail++;
        }
    };
    uint8_t out[32];
    t_sha256(out, (const uint8_t*)"abc", 3);
    expect(hex(out, 32), "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad", "sha256(abc)");
    t_sha256(out, (const uint8_t*)"", 0);
    expect(hex(out, 32), "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855", "sha256()");
    const char* two = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";  // 56 bytes: two blocks
    t_sha256(out, (const uint8_t*)two, strlen(two));
    expect(hex(out, 32), "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1", "sha256(56 bytes)");
    // RFC 6979 A.2.5: x, h1 = SHA-256("sample"), k
    uint8_t x[32], h1[32], k[32 * 4];
    unhex(x, "c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721");
    t_sha256(h1, (const uint8_t*)"sample", 6);
    t_nonce(k, x, h1, 1, 0);
    expect(hex(k, 32), "a6e3c57dd01abe90086538398355dd4c3b17aa873382b0f24d6129493d8aad60", "rfc6979 a.2.5");
    for (unsigned c = 1; c < 4; c++) {
        t_nonce(k + 32 * c, x, h1, 1, c);
        for (unsigned b = 0; b < c; b++)
            if (!memcmp(k + 32 * c, k + 32 * b, 32)) {
                printf("FAIL counters %u and %u give one nonce\n", b, c);
                fail++;
            }
    }
    if (fail) return 1;
    printf("ok\n");
    return 0;
}

// Stand-alone run of the host build of csrc/ecies_sym_dev.cuh (the streaming HMAC-SHA256 fused with the
// AES-128-CTR keystream, over csrc/aes128_dev.cuh and csrc/sha256_dev.cuh), meant to be compiled with
// ASan + UBSan and run as a child process (tests/test_ecies_sym_host.py).  Reads lines of eight fields on
// stdin:
//     mode ke km iv data s2 off_data off_s2
// mode: d (data = C, prints the message) or e (data = the message, prints C); ke 32, km 64, iv 32 hex
// digits; data and s2 hex strings, "-" when empty; off_*: 0 .. 3, the byte offset of the string inside
// its buffer.  Each input string sits in a heap block of its own that begins with the aligned dword of
// its first byte and ends with the aligned dword of its last one, and the output in a block of exactly
// its length, so a read of a dword that holds no valid byte, or a write outside the output, is a
// sanitizer report.  Prints "tag out" per line ("-" for an empty out).  A malformed line ends the run
// with exit code 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/ecies_sym_dev.cuh"

static int nib(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    out.clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        int a = nib(s[i]), b = nib(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((uint8_t)(a * 16 + b));
    }
    return true;
}

template <size_t N>
static bool words(const std::string& s, uint32_t (&w)[N]) {
    std::vector<uint8_t> b;
    if (!unhex(s, b) || b.size() != 4 * N) return false;
    for (size_t j = 0; j < N; j++)
        w[j] = ((uint32_t)b[4 * j] << 24) | ((uint32_t)b[4 * j + 1] << 16) | ((uint32_t)b[4 * j + 2] << 8) | b[4 * j + 3];
    return true;
}

// a heap block of whole dwords that holds `v` from byte `off` on and nothing behind its last dword
static uint8_t* place(const std::vector<uint8_t>& v, unsigned off) {
    size_t bytes = (off + v.size() + 3) / 4 * 4;
    uint8_t* p = (uint8_t*)malloc(bytes ? bytes : 4);
    if (!p) abort();
    memset(p, 0xEE, bytes ? bytes : 4);
    if (!v.empty()) memcpy(p + off, v.data(), v.size());
    return p;
}

int main() {
    static uint32_t te[gsv::AES_TE0_WORDS];
    for (uint32_t t = 0; t < 256; t++) gsv::aes_te0_fill(te, t);
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        std::vector<std::string> f;
        for (char* t = strtok(line, " \r\n"); t; t = strtok(nullptr, " \r\n")) f.push_back(t);
        if (f.empty()) continue;
        if (f.size() != 8 || (f[0] != "d" && f[0] != "e")) return 2;
        uint32_t ke[4], km[8], iv[4], tag[8];
        std::vector<uint8_t> data, s2;
        if (!words(f[1], ke) || !words(f[2], km) || !words(f[3], iv) || !unhex(f[4], data) || !unhex(f[5], s2)) return 2;
        unsigned od = (unsigned)atoi(f[6].c_str()), os = (unsigned)atoi(f[7].c_str());
        if (od > 3 || os > 3) return 2;
        uint8_t* bd = place(data, od);
        uint8_t* bs = place(s2, os);
        uint8_t* out = (uint8_t*)malloc(data.size() ? data.size() : 1);
        if (!out) abort();
        if (f[0] == "d")
            gsv::ecies_sym<false>(tag, ke, km, bd + od, (uint32_t)data.size(), iv, bs + os, (uint32_t)s2.size(), out, te);
        else
            gsv::ecies_sym<true>(tag, ke, km, bd + od, (uint32_t)data.size(), iv, bs + os, (uint32_t)s2.size(), out, te);
        for (int j = 0; j < 8; j++) printf("%08x", tag[j]);
        printf(" ");
        if (data.empty()) printf("-");
        for (size_t i = 0; i < data.size(); i++) printf("%02x", out[i]);
        printf("\n");
        free(bd);
        free(bs);
        free(out);
    }
    return 0;
}

// Host build of the Merkle-Damgard device headers (csrc/md_block_dev.cuh over csrc/sha256_dev.cuh and
// csrc/ripemd160_dev.cuh): a stand-alone program for tests/test_md_hash_host.py, built with g++ and, when
// they link, ASan + UBSan.  Each input line is
//     <s|r> <message hex, or - for the empty message> <offset 0-3>
// The message is copied `offset` bytes into a heap block of exactly offset + length bytes, so that it
// ends with the block and a read past its last byte is the sanitizer's to report; the program prints the
// SHA-256 digest (s) or the 20-byte RIPEMD-160 digest (r) in hex.  A malformed line exits with status 2.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../geth-sharding_amd/csrc/md_block_dev.cuh"
#include "../../geth-sharding_amd/csrc/ripemd160_dev.cuh"
#include "../../geth-sharding_amd/csrc/sha256_dev.cuh"

static int nib(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    out.clear();
    if (s == "-") return true;
    if (s.empty() || s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        int a = nib(s[i]), b = nib(s[i + 1]);
        if (a < 0 || b < 0) return false;
        out.push_back((uint8_t)(a * 16 + b));
    }
    return true;
}

static void put_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\n");
}

// a malformed line: status 2, with nothing left for the leak check to report
static int refuse(char* line) {
    free(line);
    return 2;
}

int main() {
    char* line = nullptr;
    size_t cap = 0;
    ssize_t got;
    while ((got = getline(&line, &cap, stdin)) > 0) {
        std::string ln(line, (size_t)got);
        while (!ln.empty() && (ln.back() == '\n' || ln.back() == '\r')) ln.pop_back();
        if (ln.empty()) continue;
        // three fields separated by single spaces
        size_t a = ln.find(' '), b = a == std::string::npos ? a : ln.find(' ', a + 1);
        if (a != 1 || b == std::string::npos || b + 2 != ln.size()) return refuse(line);
        const char kind = ln[0];
        const int shift = ln[b + 1] - '0';
        std::vector<uint8_t> msg;
        if ((kind != 's' && kind != 'r') || shift < 0 || shift > 3 || !unhex(ln.substr(2, b - 2), msg)) return refuse(line);
        const size_t len = msg.size();
        uint8_t* block = (uint8_t*)malloc(shift + len ? shift + len : 1);
        if (!block) return 3;
        uint8_t* p = block + shift;
        if (len) memcpy(p, msg.data(), len);
        const uint64_t nb = gsv::md_block_count(len);
        uint32_t w[16];
        if (kind == 's') {
            uint32_t s[8];
            for (int k = 0; k < 8; k++) s[k] = gsv::SHA256_IV[k];
            for (uint64_t i = 0; i < nb; i++) {
                gsv::md_load_block<true>(w, p, len, i);
                gsv::sha256_compress_inline(s, w);
            }
            uint8_t d[32];
            for (int k = 0; k < 8; k++)
                for (int t = 0; t < 4; t++) d[4 * k + t] = (uint8_t)(s[k] >> (24 - 8 * t));
            put_hex(d, 32);
        } else {
            uint32_t h[5];
            gsv::ripemd160_init(h);
            for (uint64_t i = 0; i < nb; i++) {
                gsv::md_load_block<false>(w, p, len, i);
                gsv::ripemd160_compress(h, w);
            }
            uint8_t d[20];
            for (int k = 0; k < 5; k++)
                for (int t = 0; t < 4; t++) d[4 * k + t] = (uint8_t)(h[k] >> (8 * t));
            put_hex(d, 20);
        }
        free(block);
    }
    free(line);
    return 0;
}

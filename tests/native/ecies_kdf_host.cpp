// Stand-alone run of the host build of csrc/ecies_kdf.cuh over csrc/sha256_dev.cuh, meant to be compiled
// with ASan + UBSan and run as a child process (tests/test_ecies_kdf_host.py).  Reads lines of 64 hex
// digits (a shared secret X, 32 bytes) on stdin and prints for each one line of 96 hex digits:
// Ke (16 bytes) || Km (32 bytes), the keys of ECIES_AES128_SHA256 with s1 empty.  A malformed line ends
// the run with exit code 2.
#include <cstdio>
#include <cstring>

#include "../../geth-sharding_amd/csrc/ecies_kdf.cuh"

static int nib(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        size_t len = strcspn(line, "\r\n");
        if (len == 0) continue;
        if (len != 64) return 2;
        uint32_t x[8], ke[4], km[8];
        for (int j = 0; j < 8; j++) {  // big-endian words in message order
            uint32_t w = 0;
            for (int d = 0; d < 8; d++) {
                int v = nib(line[8 * j + d]);
                if (v < 0) return 2;
                w = (w << 4) | (uint32_t)v;
            }
            x[j] = w;
        }
        gsv::ecies_kdf_keys(ke, km, x);
        for (int j = 0; j < 4; j++) printf("%08x", ke[j]);
        for (int j = 0; j < 8; j++) printf("%08x", km[j]);
        printf("\n");
    }
    return 0;
}

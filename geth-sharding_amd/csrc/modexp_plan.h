// Host side of the modexp precompile (core/vm/contracts.go:226-252), free of HIP (plain C++17;
// tests/native/modexp_host_main.cpp compiles it with g++): the 96-byte header, getData's right padding
// (core/vm/common.go:37-47), the width class of a modulus, the rows the host form stages and the size of
// the device form's work buffer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace gsv {
namespace mdx {

constexpr uint64_t MAX_LEN = 1024;  // GSV_MODEXP_MAX_LEN
constexpr int NCLASS = 6;           // modulus widths of 32, 64, 128, 256, 512, 1024 bytes
constexpr int LDS_ACC_MAX_LIMBS = 64;  // classes up to this width keep the products' accumulator in LDS
constexpr size_t MAX_WAVES = 2048;  // waves of a launch of the wide classes; each walks the items in strides

// the class of a modulus of 1 .. 1024 bytes: the smallest width that holds it
inline int width_class(uint32_t mod_len) {
    int c = 0;
    while ((32u << c) < mod_len) c++;
    return c;
}
inline uint32_t class_limbs(int c) { return 8u << c; }

// numbers a lane keeps in the work buffer (modexp_dev.cuh Slots): all six, or all but the accumulator
inline uint32_t work_slots(uint32_t limbs) { return limbs <= (uint32_t)LDS_ACC_MAX_LIMBS ? 5 : 6; }

// Bytes of work buffer for n rows with this modulus length: nothing for the 32-byte class (registers),
// else work_slots numbers of the class width per lane of each wave launched.
inline size_t waves_for(size_t n) {
    const size_t w = (n + 63) / 64;
    return w < MAX_WAVES ? w : MAX_WAVES;
}
inline size_t work_bytes(size_t n, uint32_t mod_len) {
    if (n == 0 || mod_len == 0 || mod_len > MAX_LEN) return 0;
    const int c = width_class(mod_len);
    if (c == 0) return 0;
    return waves_for(n) * 64 * work_slots(class_limbs(c)) * class_limbs(c) * 4;
}

struct Header {
    uint64_t base_len, exp_len, mod_len;
};

// new(big.Int).SetBytes(getData(input, at, 32)).Uint64(): the low 64 bits of the word, zeros past the input
inline uint64_t length_word(const uint8_t* in, size_t len, size_t at) {
    uint64_t v = 0;
    for (size_t i = at + 24; i < at + 32; i++) v = (v << 8) | (i < len ? in[i] : 0);
    return v;
}
inline Header parse_header(const uint8_t* in, size_t len) {
    return Header{length_word(in, len, 0), length_word(in, len, 32), length_word(in, len, 64)};
}
inline bool too_long(const Header& h) { return h.base_len > MAX_LEN || h.exp_len > MAX_LEN || h.mod_len > MAX_LEN; }
// an item that reaches the device: one within the cap whose output is not empty
inline bool has_work(const Header& h) { return !too_long(h) && h.mod_len != 0; }

// dst[0 .. width) = getData(body, start, size) behind width - size zero bytes (size <= width)
inline void stage_operand(uint8_t* dst, size_t width, const uint8_t* body, size_t body_len, uint64_t start,
                          uint64_t size) {
    memset(dst, 0, width);
    if (start >= body_len || size == 0) return;
    const size_t have = body_len - start < size ? body_len - start : size;
    memcpy(dst + (width - size), body + start, have);
}

// one staged row: base || exp || mod at the group's widths
inline void stage_row(uint8_t* row, uint32_t bw, uint32_t ew, uint32_t mw, const uint8_t* in, size_t len,
                      const Header& h) {
    const uint8_t* body = len > 96 ? in + 96 : in;
    const size_t blen = len > 96 ? len - 96 : 0;
    stage_operand(row, bw, body, blen, 0, h.base_len);
    stage_operand(row + bw, ew, body, blen, h.base_len, h.exp_len);
    stage_operand(row + bw + ew, mw, body, blen, h.base_len + h.exp_len, h.mod_len);
}

}  // namespace mdx
}  // namespace gsv

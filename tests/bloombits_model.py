"""Python-integer model of core/bloombits, common/bitutil's codec and bloomFilter, statement for statement.

    Generator.AddBloom / Bitset            core/bloombits/generator.go:52-87
    bitsetEncodeBytes / CompressBytes      common/bitutil/compress.go:60-97
    bitsetDecodeBytes / DecompressBytes    common/bitutil/compress.go:102-170
    NewMatcher's dropping                  core/bloombits/matcher.go:105-122
    a session's match                      core/bloombits/matcher.go:182-211, :234-238, :337-366
    bloomFilter                            eth/filters/filter.go:278-305

Pinned to the reference by tests/test_bloombits_cpu.py (the fixture tests/golden/bloombits.json and two relations of
the reference's own tests).  The GPU tests take every expected value from here.
"""
import receipt_model as R

ST_OK = 0
ST_MISSING_DATA = 37
ST_UNREFERENCED_DATA = 38
ST_EXCEEDED_TARGET = 39
ST_ZERO_CONTENT = 40
ERR_NAMES = {"errMissingData": ST_MISSING_DATA, "errUnreferencedData": ST_UNREFERENCED_DATA,
             "errExceededTarget": ST_EXCEEDED_TARGET, "errZeroContent": ST_ZERO_CONTENT, None: ST_OK}

BLOOM_BITS = 2048
BLOOM_BYTES = 256


# ---------------------------------------------------------------- generator.go
class Generator:
    def __init__(self, sections):
        if sections % 8 != 0:
            raise ValueError("section count not multiple of 8")
        self.sections = sections
        self.next_bit = 0
        self.blooms = [bytearray(sections // 8) for _ in range(BLOOM_BITS)]

    def add_bloom(self, index, bloom):
        if self.next_bit >= self.sections:
            raise ValueError("section out of bounds")
        if self.next_bit != index:
            raise ValueError("bloom filter with unexpected index")
        byte_index = self.next_bit // 8
        bit_mask = 1 << (7 - self.next_bit % 8)
        for i in range(BLOOM_BITS):
            if bloom[BLOOM_BYTES - 1 - i // 8] & (1 << (i % 8)):
                self.blooms[i][byte_index] |= bit_mask
        self.next_bit += 1

    def bitset(self, idx):
        if self.next_bit != self.sections:
            raise ValueError("bloom not fully generated yet")
        if idx >= self.sections:
            raise ValueError("section out of bounds")
        return bytes(self.blooms[idx])


def generate_sections(blooms, section_size):
    """the dense table of whole sections: bytes of n_sections x 2048 x section_size / 8"""
    assert len(blooms) % section_size == 0
    out = bytearray()
    for s in range(len(blooms) // section_size):
        g = Generator(section_size)
        for j in range(section_size):
            g.add_bloom(j, blooms[s * section_size + j])
        for rows in g.blooms:
            out += rows
    return bytes(out)


def generate_sections_np(blooms, section_size):
    """generate_sections over an (n, 256) uint8 array, as an (n_sections, 2048, section_size / 8) array: the same
    rotation stated with numpy for the sizes the loop above is too slow for (test_bloombits_cpu.py holds the two
    together).  Bloom bit i is byte 255 - i / 8 under mask 1 << (i % 8): column 2047 - i of the bits unpacked MSB
    first; block j of a vector is byte j / 8 under mask 1 << (7 - j % 8): packed MSB first."""
    import numpy as np
    n = blooms.shape[0]
    assert n % section_size == 0 and section_size % 8 == 0
    bits = np.unpackbits(np.ascontiguousarray(blooms, np.uint8), axis=1)[:, ::-1]
    return np.packbits(bits.reshape(n // section_size, section_size, BLOOM_BITS).transpose(0, 2, 1), axis=2)


# ---------------------------------------------------------------- compress.go
def bitset_encode_bytes(data):
    if len(data) == 0:
        return b""
    if len(data) == 1:
        return b"" if data[0] == 0 else bytes(data)
    non_zero_bitset = bytearray((len(data) + 7) // 8)
    non_zero_bytes = bytearray()
    for i, b in enumerate(data):
        if b != 0:
            non_zero_bytes.append(b)
            non_zero_bitset[i // 8] |= 1 << (7 - i % 8)
    if len(non_zero_bytes) == 0:
        return b""
    return bitset_encode_bytes(non_zero_bitset) + bytes(non_zero_bytes)


def compress_bytes(data):
    out = bitset_encode_bytes(data)
    return out if len(out) < len(data) else bytes(data)


class DecodeError(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def _decode_partial(data, target):
    if target == 0:
        return b"", 0
    decomp = bytearray(target)
    if len(data) == 0:
        return decomp, 0
    if target == 1:
        decomp[0] = data[0]
        return decomp, 1 if data[0] != 0 else 0
    non_zero_bitset, ptr = _decode_partial(data, (target + 7) // 8)
    for i in range(8 * len(non_zero_bitset)):
        if non_zero_bitset[i // 8] & (1 << (7 - i % 8)):
            if ptr >= len(data):
                raise DecodeError(ST_MISSING_DATA)
            if i >= len(decomp):
                raise DecodeError(ST_EXCEEDED_TARGET)
            if data[ptr] == 0:
                raise DecodeError(ST_ZERO_CONTENT)
            decomp[i] = data[ptr]
            ptr += 1
    return decomp, ptr


def bitset_decode_bytes(data, target):
    """(bytes, ST_OK) or (None, the error's status)"""
    try:
        out, size = _decode_partial(data, target)
    except DecodeError as e:
        return None, e.status
    if size != len(data):
        return None, ST_UNREFERENCED_DATA
    return bytes(out), ST_OK


def decompress_bytes(data, target):
    if len(data) > target:
        return None, ST_EXCEEDED_TARGET
    if len(data) == target:
        return bytes(data), ST_OK
    return bitset_decode_bytes(data, target)


# ---------------------------------------------------------------- matcher.go
def bloom_indexes(clause):
    """calcBloomIndexes (matcher.go:41-52) == bloom9's three bit numbers"""
    return R.bloom_indexes(bytes(clause))


def kept_rules(filters):
    """NewMatcher (matcher.go:105-122) over clauses as bytes or None: the rules that remain, clauses untouched"""
    out = []
    for rule in filters or []:
        if rule is None or len(rule) == 0:
            continue
        if any(cl is None for cl in rule):
            continue
        out.append(list(rule))
    return out


def new_matcher_filters(filters):
    return [[bloom_indexes(cl) for cl in rule] for rule in kept_rules(filters)]


def match_section(filters, rows, section_bytes):
    """matcher.go:238, :337-366 for one section: filters as bit numbers, rows(bit) -> the section's vector of `bit`"""
    acc = (1 << (8 * section_bytes)) - 1
    for rule in filters:
        any_ = 0
        for clause in rule:
            v = (1 << (8 * section_bytes)) - 1
            for bit in clause:
                v &= int.from_bytes(rows(bit & 2047), "big")
            any_ |= v
        acc &= any_
    return acc.to_bytes(section_bytes, "big")


def match_blocks(filters, rows, section_size, first_section, n_sections, begin, end):
    """the block numbers a session delivers (matcher.go:182-211) over the sections of the table; rows(section, bit)"""
    out = []
    for s in range(first_section, first_section + n_sections):
        bitset = match_section(filters, lambda bit: rows(s, bit), section_size // 8)
        start = s * section_size
        first = max(start, begin)
        last = min(start + section_size - 1, end)
        for i in range(first, last + 1):
            if bitset[(i - start) // 8] & (1 << (7 - i % 8)):
                out.append(i)
    return out


def match_bitset(filters, rows, section_size, section, begin, end):
    """one section's match bitset with the blocks outside [begin, end] cleared, and its count"""
    bitset = bytearray(match_section(filters, rows, section_size // 8))
    start = section * section_size
    for i in range(start, start + section_size):
        if not begin <= i <= end:
            bitset[(i - start) // 8] &= ~(1 << (7 - i % 8)) & 0xFF
    return bytes(bitset), sum(bin(b).count("1") for b in bitset)


# ---------------------------------------------------------------- filter.go
def bloom_lookup(bloom, item):
    return all(bloom[BLOOM_BYTES - 1 - b // 8] & (1 << (b % 8)) for b in bloom_indexes(item))


def bloom_filter(bloom, addresses, topics):
    if len(addresses) > 0:
        if not any(bloom_lookup(bloom, a) for a in addresses):
            return False
    for sub in topics:
        included = len(sub) == 0
        for t in sub:
            if bloom_lookup(bloom, t):
                included = True
                break
        if not included:
            return False
    return True


def flatten(addresses, topics):
    """filters.New (filter.go:66-80)"""
    out = []
    if len(addresses) > 0:
        out.append([bytes(a) for a in addresses])
    for sub in topics:
        out.append([bytes(t) for t in sub])
    return out


def filter_bits(filters_bits, bloom):
    """the matcher's rule evaluation over one bloom's bits (what gsv_bloom_filter_dev computes)"""
    for rule in filters_bits:
        if not any(all(bloom[BLOOM_BYTES - 1 - (b & 2047) // 8] & (1 << (b % 8)) for b in cl) for cl in rule):
            return False
    return True


# ---------------------------------------------------------------- matcher_test.go's rows
def modulo_row(bit, section, section_size):
    """generateBitset (matcher_test.go:247-259): block % bit == 0"""
    out = bytearray(section_size // 8)
    for i in range(section_size):
        if (section * section_size + i) % bit == 0:
            out[i // 8] |= 1 << (7 - i % 8)
    return bytes(out)


def exp_match3(filters, i):
    """matcher_test.go:261-286"""
    return all(any(all(i % b == 0 for b in cl) for cl in rule) for rule in filters)

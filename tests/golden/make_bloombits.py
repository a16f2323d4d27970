"""Writes tests/golden/bloombits.json: the data of the reference's own tests of the bitset codec and the matcher
(inputs, sizes, which error, filters and ranges), nothing computed.  tests/test_bloombits_cpu.py pins the model
(tests/bloombits_model.py) to it.  Run from the repository root: python tests/golden/make_bloombits.py"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# TestEncodingCycle (common/bitutil/compress_test.go:28-62): bitsetDecodeBytes(bitsetEncodeBytes(x), len(x)) == x
ENCODING_CYCLE = [
    "000000000000000000",
    "ef0400",
    "df7070533534333636313639343638373532313536346c1bc33339343837313070706336343035336336346c65fefb3930393233383838ac2f65fefb",
    "7b64000000",
    "000034000000000000",
    "0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000f0000000000000000000",
    "4912385c0e7b64000000",
    "000034000000000000000000000000000000",
    "00",
    "000003e834ff7f0000",
    "0000",
    "0000000000000000000000000000000000000000000000000000000000ff00",
    "895f0c6a020f850c6a020f85f88df88d",
    "df7070533534333636313639343638373432313536346c1bc3315aac2f65fefb",
    "0000000000",
    "df70706336346c65fefb",
    "00006d643634000000",
    "df7070533534333636313639343638373532313536346c1bc333393438373130707063363430353639343638373532313536346c1bc333393438336336346c65fe",
]

# TestDecodingCycle (:65-115): bitsetDecodeBytes(input, size) fails with `fail`, or re-encodes to the input
DECODING_CYCLE = [
    (0, "", None),
    (0, "0020", "errUnreferencedData"),
    (0, "30", "errUnreferencedData"),
    (1, "00", "errUnreferencedData"),
    (2, "07", "errMissingData"),
    (1024, "8000", "errZeroContent"),
    (29490, "343137343733323134333839373334323073333930783e3078333930783e70706336346c65303e", "errMissingData"),
    (59395, "00", "errUnreferencedData"),
    (52574, "70706336346c65c0de", "errExceededTarget"),
    (42264, "07", "errMissingData"),
    (52, "a5045bad48f4", "errExceededTarget"),
    (52574, "c0de", "errMissingData"),
    (52574, "", None),
    (29490, "34313734373332313433383937333432307333393078073034333839373334323073333930783e3078333937333432307333393078073061333930783e70706336346c65303e", "errMissingData"),
    (29491, "3973333930783e30783e", "errMissingData"),
    (1024, "808080608080", None),
    (1024, "808470705e3632383337363033313434303137393130306c6580ef46806380635a80", None),
    (1024, "8080808070", None),
    (1024, "808070705e36346c6580ef46806380635a80", None),
    (1024, "80808046802680", None),
    (1024, "4040404035", None),
    (1024, "4040bf3ba2b3f684402d353234373438373934409fe5b1e7ada94ebfd7d0505e27be4035", None),
    (1024, "404040bf3ba2b3f6844035", None),
    (1024, "40402d35323437343837393440bfd7d0505e27be4035", None),
]

# TestCompression (:119-144): CompressBytes(in) == out, DecompressBytes(out, len(in)) == in; a longer input fails
COMPRESSION = [
    ("4912385c0e7b64000000", "80fe4912385c0e7b64"),
    ("df7070533534333636313639343638373532313536346c1bc33339343837313070706336343035336336346c65fefb3930393233383838ac2f65fefb",
     "df7070533534333636313639343638373532313536346c1bc33339343837313070706336343035336336346c65fefb3930393233383838ac2f65fefb"),
]
COMPRESSION_LONG = {"input": "c00101", "size": 2, "fail": "errExceededTarget"}

# TestMatcherWildcards (core/bloombits/matcher_test.go:32-55): a clause as hex, None for a nil clause, a rule None
# for a nil rule; NewMatcher keeps 3 rules of 2, 2 and 1 clauses
ADDR0, ADDR1 = "00" * 20, "01" + "00" * 19
HASH0, HASH1 = "00" * 32, "01" + "00" * 31
WILDCARDS = {
    "filters": [[ADDR0, ADDR1], [HASH0, HASH1], [HASH1], [HASH1, None], [None, HASH1], [None, None], [], None],
    "kept": [2, 2, 1],
}

# TestMatcherContinuous (:58-62) and TestMatcherShifted (:86-96): filters as bit numbers, the range [start, blocks - 1],
# rows made as block % bit == 0 over sections of 4,096 (testSectionSize).  {32, 3125, 100} names a row outside a table
# of 2,048 rows and is left out.
MATCHER = {
    "section_size": 4096,
    "continuous": [
        {"filter": [[[10, 20, 30]]], "start": 0, "blocks": 100000},
        {"filter": [[[4, 8, 11], [7, 8, 17]], [[9, 9, 12], [15, 20, 13]], [[18, 15, 15], [12, 10, 4]]], "start": 0,
         "blocks": 10000},
    ],
    "shifted": {"filter": [[[16, 16, 16]]], "start": 9, "blocks": 64},
}


def main():
    out = {
        "encoding_cycle": ENCODING_CYCLE,
        "decoding_cycle": [{"size": s, "input": i, "fail": f} for s, i, f in DECODING_CYCLE],
        "compression": [{"in": i, "out": o} for i, o in COMPRESSION],
        "compression_long": COMPRESSION_LONG,
        "wildcards": WILDCARDS,
        "matcher": MATCHER,
    }
    path = os.path.join(HERE, "bloombits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(ENCODING_CYCLE), "inputs,", len(DECODING_CYCLE), "rows,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/receipts.json from the model (tests/receipt_model.py, tests/receipt_cases.py): a few dozen
small lists of RLP-encoded receipts with the model's bloom, receipt root, gas used and statuses, and bloom9's bit
numbers of a few byte strings.  Run from the repository root: python tests/golden/make_receipts.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import receipt_cases as C  # noqa: E402
import receipt_model as R  # noqa: E402


def entry(name, blobs):
    st, bloom, root, gas, sts = R.validate(blobs)
    return {"name": name, "receipts": [b.hex() for b in blobs], "status": st, "bloom": bloom.hex(), "root": root.hex(),
            "gas_used": gas, "receipt_status": sts}


def main():
    small = [(n, b) for n, b in C.good_shapes() if len(b) < 2000]
    lists = [entry("empty", [])]
    lists += [entry(n, [b]) for n, b in small[:12]]
    lists.append(entry("every small good shape", [b for _, b in small]))
    for k, lst in enumerate(C.random_lists(2024, [1, 2, 3, 5, 8, 13, 16, 17], max_logs=3)):
        lists.append(entry(f"random {k}", lst))
    bad = {n: b for n, b, s in C.decode_corpus() if s != R.ST_OK and len(b) < 2000}
    good = C.random_lists(7, [4], max_logs=2)[0]
    for n in ("status 02", "gas leading zero", "bytes behind the list", "empty item", "topic 31", "log of four"):
        lists.append(entry("failed: " + n, good[:2] + [bad[n]] + good[2:]))
    lists.append(entry("failed: two, the first decides", good[:1] + [bad["status 00"], bad["address 19"]] + good[1:]))
    words = [b"testtest", b"test", b"hallo", b"other", b"tes", b"lo", b"", bytes(20), bytes(32), bytes(range(135)),
             bytes(range(136)), bytes(range(137)), bytes(300)]
    out = {"lists": lists, "bloom9": [{"data": w.hex(), "indexes": R.bloom_indexes(w)} for w in words]}
    with open(os.path.join(HERE, "receipts.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(lists), "lists", os.path.getsize(os.path.join(HERE, "receipts.json")), "bytes")


if __name__ == "__main__":
    main()

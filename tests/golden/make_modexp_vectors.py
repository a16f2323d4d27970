"""Writes tests/golden/modexp_vectors.json: the name, input and expected fields of modexpTests
(core/vm/contracts_test.go:36-116 of the reference), read from the Go file's text.  Run once where the
reference is present:

    python tests/golden/make_modexp_vectors.py /path/to/reference

No test runs it; the tests read the JSON file.
"""
import json
import os
import re
import sys


def vectors(go_text):
    m = re.search(r"var modexpTests = \[\]precompiledTest\{(.*?)\n\}\n", go_text, re.S)
    body = m.group(1)
    out = []
    # one struct literal per vector; a string field is one or more "..." literals joined by +
    for item in re.split(r"\},\s*\{", body):
        f = {}
        for key in ("input", "expected", "name"):
            mm = re.search(key + r":\s*((?:\"[^\"]*\"\s*\+?\s*)+)", item)
            f[key] = "".join(re.findall(r"\"([^\"]*)\"", mm.group(1)))
        out.append(f)
    return out


def main():
    ref = sys.argv[1]
    text = open(os.path.join(ref, "core", "vm", "contracts_test.go")).read()
    v = vectors(text)
    assert len(v) == 17, len(v)
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "modexp_vectors.json")
    with open(dst, "w") as f:
        json.dump({"source": "core/vm/contracts_test.go:36-116 modexpTests", "vectors": v}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

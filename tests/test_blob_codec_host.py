"""CPU check of csrc/blob_codec.h, the per-chunk rules the kernels of csrc/blob.hip run:
tests/native/blob_codec_host.cpp (g++, with ASan + UBSan when the compiler links them; a stand-alone
program run as a child process) serializes blob lists by calling serialize_group for every 16-byte output
group through the kernel's plan tables, and deserializes bodies with index_body + strip_word.  Compared
byte for byte with the oracle's restatement of sharding/utils/marshal.go.  The plan's sizes are compared
with gsv_blob_serialized_size / gsv_proposer_body_layout of libgsv.so (host arithmetic: no GPU)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import blob_corpus as BC
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "blob_codec_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("blob_codec") / "blob_codec_host"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", str(out), SRC]
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:  # no sanitizer runtime: plain build
        subprocess.run(base, check=True)
    return str(out)


def _ser_case(lists, align):
    blobs = [b for lst in lists for b, _ in lst]
    flags = [f for lst in lists for _, f in lst]
    lo = np.cumsum([0] + [len(lst) for lst in lists]).astype("<u8")
    bo = np.cumsum([0] + [len(b) for b in blobs]).astype("<u8")
    return (struct.pack("<III", 0, align, len(lists)) + lo.tobytes() + struct.pack("<I", len(blobs)) + bo.tobytes() +
            bytes(flags) + b"".join(blobs))


def _run(exe, tmp_path, cases):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<I", len(cases)) + b"".join(cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d" % len(cases)), r.stdout
    return fout.read_bytes()


def _read_bodies(buf, pos, n):
    off = np.frombuffer(buf, "<u8", n + 1, pos)
    pos += 8 * (n + 1)
    bodies = [buf[pos + int(off[i]):pos + int(off[i + 1])] for i in range(n)]
    return off, bodies, pos + int(off[n])


def _read_blobs(buf, pos):
    (nb,) = struct.unpack_from("<I", buf, pos)
    pos += 4
    out = []
    for _ in range(nb):
        ln, sk = struct.unpack_from("<IB", buf, pos)
        out.append((buf[pos + 5:pos + 5 + ln], sk))
        pos += 5 + ln
    return out, pos


def test_serialize_matches_the_oracle(exe, tmp_path, oracle):
    sets = list(BC.list_sets().items()) + [("straddle %d" % i, [lst]) for i, lst in enumerate(BC.straddle_lists())]
    cases = [_ser_case(lists, align) for _, lists in sets for align in range(4)]
    buf = _run(exe, tmp_path, cases)
    pos = 0
    for name, lists in sets:
        want = [oracle.blob_serialize([b for b, _ in lst], [f for _, f in lst]) if lst else b"" for lst in lists]
        for align in range(4):
            off, got, pos = _read_bodies(buf, pos, len(lists))
            assert got == want, (name, align)
            assert list(off) == list(np.cumsum([0] + [len(w) for w in want])), (name, align)
    assert pos == len(buf)


def test_marshal_test_vector_bytes(exe, tmp_path):
    """sharding/utils/marshal_test.go:183-217: 60 bytes -> 00 | 0..30, 1d | 31..59 | 00 00"""
    buf = _run(exe, tmp_path, [_ser_case([BC.marshal_test_vector()], 1)])
    _, (body,), _ = _read_bodies(buf, 0, 1)
    assert body == b"\x00" + bytes(range(31)) + b"\x1d" + bytes(range(31, 60)) + b"\x00\x00"


def test_round_trip_matches_the_oracle(exe, tmp_path, oracle):
    """Deserialize(Serialize(x)) through the header's functions == the oracle's, zero-length blobs dropped"""
    lists = [lst for ls in BC.list_sets().values() for lst in ls] + BC.straddle_lists()
    bodies = [oracle.blob_serialize([b for b, _ in lst], [f for _, f in lst]) if lst else b"" for lst in lists]
    bodies += list(BC.edge_bodies().values())
    cases = [struct.pack("<IIQ", 1, i % 4, len(b)) + b for i, b in enumerate(bodies)]
    buf = _run(exe, tmp_path, cases)
    pos = 0
    for i, body in enumerate(bodies):
        got, pos = _read_blobs(buf, pos)
        assert got == oracle.blob_deserialize(body), i
        if i < len(lists):
            assert got == [(b, f) for b, f in lists[i] if len(b)], i
    assert pos == len(buf)


def _tables(lens_per_list):
    lens = [n for lst in lens_per_list for n in lst]
    bo = np.cumsum([0] + lens).astype(np.uint64)
    lo = np.cumsum([0] + [len(lst) for lst in lens_per_list]).astype(np.uint64)
    return bo, lo


def test_plan_sizes_match_the_library():
    import gsv
    for name, lists in BC.list_sets().items():
        bo, lo = _tables([[len(b) for b, _ in lst] for lst in lists])
        want = np.cumsum([0] + [sum(32 * ((len(b) + 30) // 31) for b, _ in lst) for lst in lists])
        assert list(gsv.blob_serialized_size(bo, lo)) == list(want), name
    # lists that do not start at blob 0
    bo, lo = _tables([[5, 40], [0, 31, 32]])
    assert list(gsv.blob_serialized_size(bo, lo[1:])) == [0, 96]


def test_size_limit_boundary():
    """collation.go:169-171: 32,768 chunks (2^20 bytes) pass, 32,769 do not; utils.Serialize has no limit"""
    import gsv
    from gsv import _lib
    bo, lo = _tables([[124] * 8192, [124] * 8192 + [1], [31 * 32768], [31 * 32768 + 1], []])
    assert list(gsv.blob_serialized_size(bo, lo)) == [0, 1 << 20, (2 << 20) + 32, (3 << 20) + 32, (4 << 20) + 64,
                                                      (4 << 20) + 64]
    off, st = gsv.proposer_body_layout(bo, lo)
    assert list(st) == [_lib.ST_OK, _lib.ST_BODY_TOO_LARGE, _lib.ST_OK, _lib.ST_BODY_TOO_LARGE, _lib.ST_OK]
    assert list(off) == [0, 1 << 20, 1 << 20, 2 << 20, 2 << 20, 2 << 20]


def test_data_layout():
    import gsv
    off = np.array([0, 0, 31, 32, 96, 96 + 33 * 32 + 5], np.uint64)
    assert list(gsv.blob_data_layout(off)) == [0, 0, 0, 0, 64, 64 + 1024]

"""GPU check that a host form reads a caller's offset table relative to its first entry: the same items
behind a 5-byte prefix, with a table that starts at 5, give what they give packed from 0.  The package's
_pack always starts its tables at 0, so these calls go through _lib.load() directly.  The expected values
are the zero-based call's; the oracle comparisons of each entry are in its own GPU test."""
import ctypes

import numpy as np
import pytest

import block_header_cases as C
import block_header_model as B
from conftest import golden

pytestmark = pytest.mark.gpu

N = 3
BASE = 5
G1 = (1).to_bytes(32, "big") + (2).to_bytes(32, "big")  # the generator of BN254 G1


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _packed(items, base):
    """(flat, off): the items behind `base` bytes of junk, the table starting at `base`"""
    off = np.full(len(items) + 1, base, np.uint64)
    off[1:] += np.cumsum([len(m) for m in items], dtype=np.uint64)
    flat = np.frombuffer(b"\xa5" * base + b"".join(items) + b"\0" * 8, np.uint8).copy()
    return flat, off


def _hash_items(ctx):
    return [bytes(range(200)), b"", b"abc"]  # more than one Keccak / SHA block, empty, short


def _ecrecover_items(ctx):
    msg, sig, _, _ = ctx.synth_sign(seed=77, n=2, want_pub=False, want_addr=False)
    rec = [msg[i].tobytes() + bytes(31) + bytes([27 + sig[i, 64]]) + sig[i, :64].tobytes() for i in range(2)]
    return [rec[0], b"", rec[1] + b"\x01\x02\x03"]  # exact, empty (all padding), bytes past 128 ignored


def _pubkey_items(ctx):
    _, _, pub, _ = ctx.synth_sign(seed=78, n=2, want_pub=True, want_addr=False)
    compressed = bytes([2 + (pub[1, 64] & 1)]) + pub[1, 1:33].tobytes()
    return [pub[0].tobytes(), b"", compressed]


def _tx_items(ctx):
    rows = [r for r in golden("tx_sign.json")["rows"] if r["status"] == 0 and r["signer"] == 0 and r["chain_id"] == "0x1"]
    signed = sorted({bytes.fromhex(r["signed"]) for r in rows}, key=len)
    assert len(signed[0]) != len(signed[-1])
    return [signed[0], b"", signed[-1]]


def _header_items(ctx):
    blobs = sorted({B.encode_header(h) for h in C.length_sweep()}, key=len)
    assert len(blobs[0]) != len(blobs[-1])
    return [blobs[0], b"", blobs[-1]]


def _outs(*widths):
    return [np.zeros((N, w), np.uint8) for w in widths]


def _simple(name, *widths):
    def call(L, h, flat, off):
        outs = _outs(*widths)
        rc = getattr(L, name)(h, _ptr(flat), _ptr(off), N, *[_ptr(o) for o in outs])
        return rc, outs
    return call


def _tx_sender(L, h, flat, off):
    outs = _outs(20, 1)
    cid = np.frombuffer(b"\x01\0", np.uint8).copy()
    rc = L.gsv_tx_sender_batch(h, _ptr(flat), _ptr(off), N, _ptr(cid), 1, 0, _ptr(outs[0]), _ptr(outs[1]))
    return rc, outs


ENTRIES = {
    "gsv_keccak256_batch": (_hash_items, _simple("gsv_keccak256_batch", 32)),
    "gsv_sha256_batch": (_hash_items, _simple("gsv_sha256_batch", 32)),
    "gsv_ripemd160_batch": (_hash_items, _simple("gsv_ripemd160_batch", 32)),
    "gsv_ecrecover_precompile_batch": (_ecrecover_items, _simple("gsv_ecrecover_precompile_batch", 32, 1)),
    "gsv_bn256_add_batch": (lambda ctx: [G1 + G1, b"", G1], _simple("gsv_bn256_add_batch", 64, 1)),
    "gsv_bn256_scalar_mul_batch": (lambda ctx: [G1 + (7).to_bytes(32, "big"), b"", G1 + b"\x05" * 6],
                                   _simple("gsv_bn256_scalar_mul_batch", 64, 1)),
    "gsv_pubkey_parse_batch": (_pubkey_items, _simple("gsv_pubkey_parse_batch", 65, 1)),
    "gsv_tx_sender_batch": (_tx_items, _tx_sender),
    "gsv_block_header_hash_batch": (_header_items, _simple("gsv_block_header_hash_batch", 32, 32, 1)),
}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_table_with_nonzero_first_entry(ctx, name):
    from gsv import _lib
    items, call = ENTRIES[name]
    items = items(ctx)
    assert len(items) == N and len({len(m) for m in items}) == N and b"" in items
    L = _lib.load()
    rc0, want = call(L, ctx.handle, *_packed(items, 0))
    rc5, got = call(L, ctx.handle, *_packed(items, BASE))
    assert rc0 == 0 and rc5 == 0, (rc0, rc5)
    assert any(w.any() for w in want), "the zero-based call wrote nothing"
    for k, (w, g) in enumerate(zip(want, got)):
        assert (w == g).all(), (name, "output", k, w.tolist(), g.tolist())

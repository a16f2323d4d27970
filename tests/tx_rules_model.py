"""TEST INFRASTRUCTURE — a pure-Python model of the reference's transaction decode and signer rules,
written from the reference's Go text (file:line in the comments) and independent of the three decoders
under test (oracle/gsv_oracle.c tx_decode, csrc/tx_host.hip tx_prepare, csrc/notary.hip k_notary_tx):
no ctypes, no import of `oracle` or `gsv`, Python big integers throughout.

  Stream            rlp/decode.go:593-1034   Kind / readKind / readUint / readFull / willRead, Bytes, uint,
                                             List, ListEnd, with the list stack and the input limit
  decode_txdata     rlp/decode.go:136-146 DecodeBytes, :432-452 makeStructDecoder over
                    core/types/transaction.go:55-70 txdata (Hash is tagged "-")
  sender_inputs     core/types/transaction_signing.go:127-137, 155-165, 182-184, 207-220, 222-235, 250-260,
                    core/types/transaction.go:117-133, crypto/crypto.go:181-192
  deserialize       sharding/utils/marshal.go:144-198

The elliptic-curve recovery is not modelled: `sender_inputs` stops where recoverPlain calls
crypto.Ecrecover and hands back the sighash preimage and (r, s, v) for it.
"""
from __future__ import annotations

ST_OK, ST_RECOVER_FAILED, ST_INVALID_SIG, ST_INVALID_CHAIN_ID, ST_BAD_RLP = 0, 4, 5, 6, 8
SIGNER_EIP155, SIGNER_HOMESTEAD, SIGNER_FRONTIER = 0, 1, 2

BYTE, STRING, LIST = 0, 1, 2  # rlp/decode.go:555-559
U64 = (1 << 64) - 1

# crypto/crypto.go:38-39 (secp256k1N, secp256k1halfN = N / 2)
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SECP_HALF_N = SECP_N // 2


class RLPError(Exception):
    """An error value of rlp/decode.go:33-55 (or a decodeError message), by the reference's name."""

    def __init__(self, name):
        super().__init__(name)
        self.name = name


class Stream:
    """rlp/decode.go:593-608.  `limit` None is a reader without an input limit (Reset, :824-841)."""

    def __init__(self, data: bytes, limit="len"):
        self.data, self.rpos = bytes(data), 0
        if limit == "len":  # bytes.Reader: the limit is discovered (:831-834) or passed (DecodeBytes :139)
            limit = len(data)
        self.limited = limit is not None
        self.remaining = limit if self.limited else 0
        self.stack = []  # [pos, size] per open list
        self.kind, self.size, self.byteval, self.kinderr = -1, 0, 0, None

    # ---- :1016-1034
    def will_read(self, n):
        self.kind = -1  # rearm Kind
        if self.stack:
            tos = self.stack[-1]
            if n > tos[1] - tos[0]:
                raise RLPError("ErrElemTooLarge")
            tos[0] += n
        if self.limited:
            if n > self.remaining:
                raise RLPError("ErrValueTooLarge")
            self.remaining -= n

    # ---- :1005-1014
    def read_byte(self):
        self.will_read(1)
        if self.rpos >= len(self.data):
            raise RLPError("io.ErrUnexpectedEOF")
        b = self.data[self.rpos]
        self.rpos += 1
        return b

    # ---- :990-1003
    def read_full(self, n):
        self.will_read(n)
        if self.rpos + n > len(self.data):
            self.rpos = len(self.data)
            raise RLPError("io.ErrUnexpectedEOF")
        b = self.data[self.rpos:self.rpos + n]
        self.rpos += n
        return b

    # ---- :964-988
    def read_uint(self, size):
        if size == 0:
            self.kind = -1
            return 0
        if size == 1:
            return self.read_byte()
        b = self.read_full(size)
        if b[0] == 0:
            raise RLPError("ErrCanonSize")  # callers decoding integers turn this into ErrCanonInt
        return int.from_bytes(b, "big")

    # ---- :902-962
    def read_kind(self):
        try:
            b = self.read_byte()
        except RLPError as e:
            if not self.stack and e.name in ("io.ErrUnexpectedEOF", "ErrValueTooLarge"):
                raise RLPError("io.EOF")
            raise
        self.byteval = 0
        if b < 0x80:
            self.byteval = b
            return BYTE, 0
        if b < 0xB8:
            return STRING, b - 0x80
        if b < 0xC0:
            size = self.read_uint(b - 0xB7)
            if size < 56:
                raise RLPError("ErrCanonSize")
            return STRING, size
        if b < 0xF8:
            return LIST, b - 0xC0
        size = self.read_uint(b - 0xF7)
        if size < 56:
            raise RLPError("ErrCanonSize")
        return LIST, size

    # ---- :869-900.  Returns (kind, size) or raises; the error of the last readKind is sticky.
    def Kind(self):
        tos = self.stack[-1] if self.stack else None
        if self.kind < 0:
            self.kinderr = None
            if tos is not None and tos[0] == tos[1]:
                raise RLPError("EOL")
            try:
                self.kind, self.size = self.read_kind()
            except RLPError as e:
                # Go assigns all three results; kind/size are zero values beside an error
                self.kind, self.size, self.kinderr = BYTE, 0, e.name
            if self.kinderr is None:
                if tos is None:
                    if self.limited and self.size > self.remaining:
                        self.kinderr = "ErrValueTooLarge"
                elif self.size > tos[1] - tos[0]:
                    self.kinderr = "ErrElemTooLarge"
        if self.kinderr is not None:
            raise RLPError(self.kinderr)
        return self.kind, self.size

    # ---- :648-669
    def Bytes(self):
        kind, size = self.Kind()
        if kind == BYTE:
            self.kind = -1
            return bytes([self.byteval])
        if kind == STRING:
            b = self.read_full(size)
            if size == 1 and b[0] < 128:
                raise RLPError("ErrCanonSize")
            return b
        raise RLPError("ErrExpectedString")

    # ---- :703-734
    def uint(self, maxbits=64):
        kind, size = self.Kind()
        if kind == BYTE:
            if self.byteval == 0:
                raise RLPError("ErrCanonInt")
            self.kind = -1
            return self.byteval
        if kind == STRING:
            if size > maxbits // 8:
                raise RLPError("errUintOverflow")
            try:
                v = self.read_uint(size)
            except RLPError as e:
                if e.name == "ErrCanonSize":
                    raise RLPError("ErrCanonInt")
                raise
            if size > 0 and v < 128:
                raise RLPError("ErrCanonSize")
            return v
        raise RLPError("ErrExpectedString")

    # ---- :757-769
    def List(self):
        kind, size = self.Kind()
        if kind != LIST:
            raise RLPError("ErrExpectedList")
        self.stack.append([0, size])
        self.kind, self.size = -1, 0
        return size

    # ---- :773-788
    def ListEnd(self):
        if not self.stack:
            raise RLPError("errNotInList")
        tos = self.stack[-1]
        if tos[0] != tos[1]:
            raise RLPError("errNotAtEOL")
        self.stack.pop()
        if self.stack:
            self.stack[-1][0] += tos[1]
        self.kind, self.size = -1, 0


# ---------------------------------------------------------------- typed decoders
def decode_uint(s: Stream, bits=64):  # decodeUint :239-247
    return s.uint(bits)


def decode_bigint(s: Stream):  # decodeBigInt :271-287: any length, no leading zero byte
    b = s.Bytes()
    if len(b) > 0 and b[0] == 0:
        raise RLPError("ErrCanonInt")
    return int.from_bytes(b, "big")


def decode_bytes(s: Stream):  # decodeByteSlice :386-393
    return s.Bytes()


def decode_byte_array(s: Stream, vlen: int):  # decodeByteArray :395-430
    kind, size = s.Kind()
    if kind == BYTE:
        if vlen == 0:
            raise RLPError("input string too long")
        if vlen > 1:
            raise RLPError("input string too short")
        return bytes([s.uint()])
    if kind == STRING:
        if vlen < size:
            raise RLPError("input string too long")
        if vlen > size:
            raise RLPError("input string too short")
        b = s.read_full(vlen)
        if size == 1 and b[0] < 128:
            raise RLPError("ErrCanonSize")
        return b
    raise RLPError("ErrExpectedString")


def decode_optional_byte_array(s: Stream, vlen=20):
    """makeOptionalPtrDecoder :480-507 over *[vlen]byte: size 0 of string OR list kind is nil."""
    try:
        kind, size = s.Kind()
    except RLPError:
        s.kind = -1
        raise
    if size == 0 and kind != BYTE:
        s.kind = -1  # rearm: the header was consumed, nothing else is read
        return None
    return decode_byte_array(s, vlen)


def decode_txdata(blob: bytes):
    """rlp.DecodeBytes(blob, &tx) -> dict of the nine fields, or raises RLPError.
    Transaction.DecodeRLP (transaction.go:141-149) decodes into txdata through makeStructDecoder
    (decode.go:437-450): List, each field in order (EOL -> "too few elements"), ListEnd
    (errNotAtEOL -> "too many elements"); DecodeBytes refuses trailing input (:142-144)."""
    s = Stream(blob, len(blob) if len(blob) else "len")
    s.List()
    tx = {}
    fields = (("nonce", decode_uint), ("price", decode_bigint), ("gas", decode_uint),
              ("to", decode_optional_byte_array), ("value", decode_bigint), ("data", decode_bytes),
              ("v", decode_bigint), ("r", decode_bigint), ("s", decode_bigint))
    for name, dec in fields:
        try:
            tx[name] = dec(s)
        except RLPError as e:
            if e.name == "EOL":
                raise RLPError("too few elements")
            raise
    s.ListEnd()
    if s.rpos < len(s.data):
        raise RLPError("ErrMoreThanOneValue")
    return tx


# ---------------------------------------------------------------- encoding (rlp/encode.go)
def enc_head(size, small, large):  # puthead :150-162
    if size < 56:
        return bytes([small + size])
    lb = size.to_bytes((size.bit_length() + 7) // 8, "big")
    return bytes([large + len(lb)]) + lb


def enc_string(b: bytes):  # encodeString :201-210
    if len(b) == 1 and b[0] <= 0x7F:
        return bytes(b)
    return enc_head(len(b), 0x80, 0xB7) + bytes(b)


def enc_uint(i: int):  # writeUint :390-407, writeBigInt :429-438: 0 -> 0x80, < 128 -> itself
    if i == 0:
        return b"\x80"
    return enc_string(i.to_bytes((i.bit_length() + 7) // 8, "big"))


def enc_list(payload: bytes):  # listEnd / headsize: 0xC0 / 0xF7 heads
    return enc_head(len(payload), 0xC0, 0xF7) + payload


def sighash_preimage(tx, chain_id=None):
    """The bytes rlpHash (core/types/block.go:130-135) hashes for EIP155Signer.Hash (:155-165, chain_id
    given) or FrontierSigner.Hash (:207-216), re-encoded from the decoded values.  A nil *Address encodes
    as 0x80 (makePtrWriter's nilfunc for byte arrays, encode.go:552-559)."""
    p = (enc_uint(tx["nonce"]) + enc_uint(tx["price"]) + enc_uint(tx["gas"]) +
         (b"\x80" if tx["to"] is None else enc_string(tx["to"])) + enc_uint(tx["value"]) + enc_string(tx["data"]))
    if chain_id is not None:
        p += enc_uint(chain_id) + enc_uint(0) + enc_uint(0)
    return enc_list(p)


# ---------------------------------------------------------------- signers
def is_protected_v(V):  # transaction.go:126-133
    if V.bit_length() <= 8:
        return V not in (27, 28)
    return True


def derive_chain_id(V):  # transaction_signing.go:250-260
    if V.bit_length() <= 64:
        if V in (27, 28):
            return 0
        return ((V - 35) & U64) // 2  # uint64 arithmetic wraps below 35
    return (V - 35) // 2


def sender_inputs(tx, signer, chain_id):
    """types.Sender up to the call of crypto.Ecrecover.  Returns a dict:
      status   ST_OK (go on to Ecrecover with pre, r, s, v) / ST_INVALID_CHAIN_ID / ST_INVALID_SIG
      pre      sighash preimage (absent on ST_INVALID_CHAIN_ID)
      vprime   the V handed to recoverPlain (may be negative), r, s the big integers
      v        recovery id byte, when status is ST_OK
      homestead"""
    V, out = tx["v"], {"r": tx["r"], "s": tx["s"]}
    if signer == SIGNER_EIP155 and is_protected_v(V):  # :127-137
        if derive_chain_id(V) != chain_id:
            out["status"] = ST_INVALID_CHAIN_ID
            return out
        vp = V - 2 * chain_id - 8
        out["pre"] = sighash_preimage(tx, chain_id)
        homestead = True
    else:  # HomesteadSigner :182-184 (also EIP155Signer on an unprotected tx, :128-130), Frontier :218-220
        vp = V
        out["pre"] = sighash_preimage(tx)
        homestead = signer != SIGNER_FRONTIER
    out["vprime"], out["homestead"] = vp, homestead
    # recoverPlain :222-229.  big.Int.BitLen and Uint64 work on the absolute value
    if abs(vp).bit_length() > 8:
        out["status"] = ST_INVALID_SIG
        return out
    v = ((abs(vp) & U64) - 27) & 0xFF
    r, s = tx["r"], tx["s"]
    # ValidateSignatureValues crypto.go:181-192
    ok = r >= 1 and s >= 1 and not (homestead and s > SECP_HALF_N) and r < SECP_N and s < SECP_N and v in (0, 1)
    out["status"] = ST_OK if ok else ST_INVALID_SIG
    out["v"] = v
    return out


def tx_verdict(blob, signer, chain_id):
    """(status, dict): ST_BAD_RLP with the error's name, or sender_inputs' result."""
    try:
        tx = decode_txdata(blob)
    except RLPError as e:
        return ST_BAD_RLP, {"status": ST_BAD_RLP, "error": e.name}
    out = sender_inputs(tx, signer, chain_id)
    out["tx"] = tx
    return out["status"], out


# ---------------------------------------------------------------- blob codec
def deserialize(data: bytes):
    """utils.Deserialize, sharding/utils/marshal.go:144-198, literally -> [(blob bytes, skip_evm)].
    A trailing partial chunk is ignored (:145), the length is indicator & 0x1F (:132-134), skipEvm is
    bit 7 of the terminal chunk's indicator (:126-128, :185), trailing non-terminal chunks are dropped."""
    chunks = len(data) // 32
    blobs, parts = [], 0
    for i in range(chunks):
        n = data[i * 32] & 0x1F
        if n == 0:
            parts += 1
        else:
            blobs.append((parts, n))
            parts = 0
    out, cur = [], 0
    for nonterm, tl in blobs:
        b = bytearray()
        for _ in range(nonterm):
            b += data[cur + 1:cur + 32]
            cur += 32
        skip = ((data[cur] & 0x80) >> 7) == 1
        b += data[cur + 1:cur + tl + 1]
        cur += 32
        out.append((bytes(b), skip))
    return out


def serialize(blobs, skip_evm=None):
    """utils.Serialize, marshal.go:71-123 (empty blobs produce no chunk, getNumChunks :54-57)."""
    out = bytearray()
    for k, b in enumerate(blobs):
        n = (len(b) + 30) // 31
        for j in range(n):
            if j != n - 1:
                out.append(0)
                out += b[j * 31:(j + 1) * 31]
            else:
                tl = len(b) - (n - 1) * 31
                out.append(tl | (0x80 if skip_evm and skip_evm[k] else 0))
                out += b[j * 31:] + bytes(31 - tl)
    return bytes(out)

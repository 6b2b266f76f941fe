"""The specification of keyed MED-PEE (include/codec_tcc_aead.h) in pure Python
integers: ChaCha20 and Poly1305 as RFC 8439 defines them and the layout the codec lays over them.
Nothing here is shared with the product; tests compare the kernels with it bit for bit, and
tests/golden/aead_kat.json (written with the openssl binary, tests/golden/make_aead_kat.py) pins
this file in turn.

Layout.  A caller gives a 32-byte key and an 8-byte nonce; slice b of a call has the global index
g = index0 + b.
  nonce12 = LE32(g) || nonce
  otk     = ChaCha20(key, counter 0, nonce12)[0:32]          (r clamped, s as RFC 8439 §2.5)
  CT      = PT xor keystream(counter 1, 2, ...) on the first L bits of the row, zero past L;
            bit i of a row is bit i % 64 of (64-bit) word i / 64, so keystream byte k meets
            bits 8k .. 8k+7
  nb      = ceil(L / 8)
  tag     = Poly1305(otk, pad16(AAD) || pad16(CT[0:nb]) || LE64(len AAD) || LE64(nb))
A volume's stream is one row with an empty AAD at the reserved index STREAM_INDEX.
"""
MASK32 = 0xFFFFFFFF
P1305 = (1 << 130) - 5
STREAM_INDEX = 0x80000000


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & MASK32


def _quarter(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & MASK32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & MASK32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & MASK32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & MASK32; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key: bytes, counter: int, nonce12: bytes) -> bytes:
    """RFC 8439 §2.3: the 64-byte block of (key, 32-bit counter, 96-bit nonce)."""
    if len(key) != 32 or len(nonce12) != 12 or not 0 <= counter <= MASK32:
        raise ValueError("chacha20_block takes a 32-byte key, a 32-bit counter and a 12-byte nonce")
    le = lambda b, i: int.from_bytes(b[4 * i:4 * i + 4], "little")
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574] + [le(key, i) for i in range(8)] + \
           [counter] + [le(nonce12, i) for i in range(3)]
    x = list(init)
    for _ in range(10):
        _quarter(x, 0, 4, 8, 12); _quarter(x, 1, 5, 9, 13); _quarter(x, 2, 6, 10, 14); _quarter(x, 3, 7, 11, 15)
        _quarter(x, 0, 5, 10, 15); _quarter(x, 1, 6, 11, 12); _quarter(x, 2, 7, 8, 13); _quarter(x, 3, 4, 9, 14)
    return b"".join(((x[i] + init[i]) & MASK32).to_bytes(4, "little") for i in range(16))


def keystream(key: bytes, nonce12: bytes, counter0: int, nbytes: int) -> bytes:
    """nbytes of keystream from block counter0 on (the counter never wraps: ValueError)."""
    nblk = (nbytes + 63) // 64
    if counter0 + nblk > 1 << 32:
        raise ValueError("the block counter would wrap")
    return b"".join(chacha20_block(key, counter0 + i, nonce12) for i in range(nblk))[:nbytes]


def poly1305(otk: bytes, msg: bytes) -> bytes:
    """RFC 8439 §2.5: the 16-byte tag of msg under the 32-byte one-time key."""
    if len(otk) != 32:
        raise ValueError("poly1305 takes a 32-byte one-time key")
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(otk[16:], "little")
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P1305
    return ((h + s) & ((1 << 128) - 1)).to_bytes(16, "little")


def poly1305_pre_final(otk: bytes, msg: bytes) -> int:
    """The accumulator in [0, p) before s is added (tests build messages that put the kernel's
    partially reduced accumulator near p)."""
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    h = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P1305
    return h


# ------------------------------------------------------------------ the codec's layout
def check_index(g: int):
    if not (0 <= g < (1 << 31) or g == STREAM_INDEX):
        raise ValueError("slice indices are < 2^31 (0x80000000 is the volume stream's)")


def nonce12(g: int, nonce: bytes) -> bytes:
    if len(nonce) != 8:
        raise ValueError("the nonce has 8 bytes")
    check_index(g)
    return g.to_bytes(4, "little") + nonce


def one_time_key(key: bytes, g: int, nonce: bytes) -> bytes:
    return chacha20_block(key, 0, nonce12(g, nonce))[:32]


def row_bytes(words, L: int) -> bytes:
    """The first ceil(L / 8) bytes of a row of 64-bit words, bits at and past L cleared."""
    nb = (L + 7) // 8
    raw = b"".join((int(w) & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little") for w in words)
    if nb > len(raw):
        raise ValueError(f"{L} bits do not fit a row of {len(raw)} bytes")
    out = bytearray(raw[:nb])
    if L % 8:
        out[-1] &= (1 << (L % 8)) - 1
    return bytes(out)


def bytes_row(data: bytes, row_words: int):
    """data zero-padded to a row of row_words 64-bit words (list of ints)."""
    raw = data + bytes(8 * row_words - len(data))
    return [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(row_words)]


def crypt_row(key: bytes, nonce: bytes, g: int, words, L: int):
    """The row's first L bits xor the keystream of slice g from counter 1 on; zero past L.  Its
    own inverse.  Returns a list of len(words) 64-bit ints."""
    if not 0 <= L <= min(64 * len(words), (1 << 31) - 1):
        raise ValueError("L must lie in the row and below 2^31")
    pt = row_bytes(words, L)
    ks = keystream(key, nonce12(g, nonce), 1, len(pt))
    ct = bytearray(a ^ b for a, b in zip(pt, ks))
    if L % 8:
        ct[-1] &= (1 << (L % 8)) - 1
    return bytes_row(bytes(ct), len(words))


def pad16(b: bytes) -> bytes:
    return b + bytes(-len(b) % 16)


def mac_data(aad: bytes, ct: bytes) -> bytes:
    return pad16(aad) + pad16(ct) + len(aad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")


def tag_otk(otk: bytes, aad: bytes, ct_words, L: int) -> bytes:
    """The tag of (aad, the first L bits of the row) under a given one-time key."""
    return poly1305(otk, mac_data(aad, row_bytes(ct_words, L) if L else b""))


def tag(key: bytes, nonce: bytes, g: int, aad: bytes, ct_words, L: int) -> bytes:
    return tag_otk(one_time_key(key, g, nonce), aad, ct_words, L)


def tag_words(t: bytes):
    """A 16-byte tag as the four little-endian 32-bit words the kernels write."""
    return [int.from_bytes(t[4 * i:4 * i + 4], "little") for i in range(4)]


def release(key: bytes, nonce: bytes, g: int, tag_got: bytes, tag_want: bytes, ct_words, L: int):
    """(ok, plaintext row): the row decrypted when the tags agree, else all zeros."""
    ok = int(tag_got == tag_want)
    return ok, (crypt_row(key, nonce, g, ct_words, L) if ok else [0] * len(ct_words))

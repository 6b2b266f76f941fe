"""Scalar restatement of keyed blind MED-PEE: plain Python loops and ints, built on the scalar
restatement of the blind format (tests/pee_blind_scalar.py) and written from the header of
tests/pee_blind_keyed_spec.py -- the framing, the bit order and the flag are restated here with no
numpy and no helper shared with that spec.  The cipher is tests/aead_spec.py's, which openssl
vectors pin (tests/golden/aead_kat.json).  Test infrastructure: it cross-checks the spec and
generates the known answers (tests/golden/make_pee_blind_keyed_golden.py).  Images are lists of rows
of ints, bits lists of ints.
"""
from __future__ import annotations

import aead_spec as AS
import pee_blind_scalar as S

FRAME_BITS = 224
FLAG_BIT = 41   # side bit of flag bit 1: word 1 (bits 32..63), bit 8 + 1


def cover_bytes(img, nbytes: int) -> bytes:
    raw = bytearray()
    for row in img:
        for v in row:
            raw += int(v).to_bytes(nbytes, "little")
    return bytes(raw)


def _words(bits):
    out = [0] * max(1, (len(bits) + 63) // 64)
    for i, b in enumerate(bits):
        out[i // 64] |= (int(b) & 1) << (i % 64)
    return out


def user_bits(img, bits, nbytes: int, key: bytes, nonce: bytes, g: int):
    """(frame || CT as a list of bits, tag)"""
    n = len(bits)
    ct = AS.crypt_row(key, nonce, g, _words(bits), n)
    tag = AS.tag(key, nonce, g, cover_bytes(img, nbytes), ct, n)
    frame = g.to_bytes(4, "little") + nonce + tag
    out = []
    for byte in frame:
        for j in range(8):
            out.append((byte >> j) & 1)
    assert len(out) == FRAME_BITS
    for i in range(n):
        out.append((ct[i // 64] >> (i % 64)) & 1)
    return out, tag


def embed(img, bits, T: int, maxval: int, nbytes: int, key: bytes, nonce: bytes, g: int = 0, max_entries: int = 256):
    """(stego, info, tag): info = (status, n_user with the frame, E, n_side, end, region row)."""
    H, W = len(img), len(img[0])
    user, tag = user_bits(img, bits, nbytes, key, nonce, g)
    stego, info = S.embed(img, user, T, maxval, nbytes, False, max_entries)
    if info[0] == 0:
        flat = H * W - 1 - FLAG_BIT
        stego[flat // W][flat % W] |= 1
    return stego, info, tag


def choose(img, n_ct: int, tmax: int, maxval: int, max_entries: int = 256) -> int:
    for T in range(1, tmax + 1):
        if S.plan(img, FRAME_BITS + n_ct, T, maxval, max_entries)[0] == 0:
            return T
    return 0


def capacity(img, T: int, maxval: int, max_entries: int = 256) -> int:
    """The largest n_ct embed() accepts, by trying the lengths in turn (-1: not even the frame fits)."""
    n = 0
    while S.plan(img, FRAME_BITS + n, T, maxval, max_entries)[0] == 0:
        n += 1
    return n - 1


def decode(stego, nbytes: int, key: bytes):
    """(payload bits, cover, (g, nonce, tag)); ValueError without a keyed header or when the tag fails."""
    H, W = len(stego), len(stego[0])
    if H * W < 192 or S._word(stego, 0) != S.MAGIC:
        raise ValueError("no header")
    flags = (S._word(stego, 1) >> 8) & 0xFF
    if flags != 2 or S._word(stego, 2) < FRAME_BITS:
        raise ValueError("no keyed header")
    plain = [list(r) for r in stego]
    flat = H * W - 1 - FLAG_BIT
    plain[flat // W][flat % W] &= ~1
    user, cover, _hdr = S.decode(plain)
    frame = bytearray(28)
    for i in range(FRAME_BITS):
        frame[i // 8] |= user[i] << (i % 8)
    g, nonce, tag = int.from_bytes(frame[:4], "little"), bytes(frame[4:12]), bytes(frame[12:])
    ct_bits = user[FRAME_BITS:]
    ct = _words(ct_bits)
    if AS.tag(key, nonce, g, cover_bytes(cover, nbytes), ct, len(ct_bits)) != tag:
        raise ValueError("tag mismatch")
    pt = AS.crypt_row(key, nonce, g, ct, len(ct_bits))
    return [(pt[i // 64] >> (i % 64)) & 1 for i in range(len(ct_bits))], cover, (g, nonce, tag)

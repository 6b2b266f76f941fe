"""Specification of keyed blind MED-PEE (include/codec_tcc_blind_keyed.h): a blind stego
whose user bits are a 224-bit frame and a ciphertext, so that a 32-byte key is all a reader needs
besides the pixels.  TEST INFRASTRUCTURE ONLY, and a composition: the blind format is
tests/pee_blind_spec.py's (BS), the cipher tests/aead_spec.py's (AS); neither is changed.  The
kernels are checked bit-exact against embed() / decode(), and those against the scalar restatement
tests/pee_blind_keyed_scalar.py.

  slice      g = index0 + b, the slice's global index; nonce12 = LE32(g) || nonce (8 bytes)
  CT         the payload row's first n_ct bits xor the keystream of (key, nonce12), counter 1.. (AS.crypt_row)
  tag        AS.tag(key, nonce, g, the cover's bytes as they lie in memory, CT, n_ct)
  frame      nonce12 || tag, 28 bytes; byte k occupies user bits 8k .. 8k+7, LSB first
  user bits  frame (224 bits) || CT (n_ct bits): header n_user = 224 + n_ct
  embed      BS.embed(cover, user bits, T, checksum=False), then, on a slice with status 0, side
             bit 41 = 1 (flag bit 1 of header word 1: bit 0 of the pixel with flat index H W - 1 - 41)
  capacity   BS.capacity - 224, or -1 when that is negative
  auto       the smallest T in 1..tmax whose BS.plan for 224 + n_ct has status 0 (0: none; the
             slice is then refused with the plan of tmax)
  decode     flags == 2 and n_user >= 224 (ValueError otherwise); BS's decode rules with that flag
             admitted; frame -> (g, nonce, tag); AS.release under the tag of (restored cover, CT)
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

try:   # with tests/ on the path or as tests.pee_blind_keyed_spec
    import aead_spec as AS
    import pee_blind_spec as BS
except ImportError:   # pragma: no cover
    from tests import aead_spec as AS
    from tests import pee_blind_spec as BS

FLAG_KEYED = 2
FRAME_BITS = 224
FLAG_SIDE_BIT = 32 + 8 + 1   # word 1, bit 8 + 1


class TagMismatch(ValueError):
    """The tag of (restored cover, ciphertext) differs from the frame's."""


def aad(cover: np.ndarray) -> bytes:
    return np.ascontiguousarray(cover).astype(cover.dtype.newbyteorder("<"), copy=False).tobytes()


def _row(bits: np.ndarray):
    """0/1 vector -> list of 64-bit words, LSB first (at least one word)."""
    nw = max(1, (bits.size + 63) // 64)
    raw = np.zeros(8 * nw, np.uint8)
    if bits.size:
        p = np.packbits(bits, bitorder="little")
        raw[:p.size] = p
    return [int(v) for v in raw.view("<u8")]


def _bits(data: bytes, n: int) -> np.ndarray:
    return np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")[:n]


def seal(cover: np.ndarray, bits, key: bytes, nonce: bytes, g: int) -> Tuple[np.ndarray, bytes]:
    """(user bits = frame || CT, tag) of one slice."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    n = int(bits.size)
    ct = AS.crypt_row(key, nonce, g, _row(bits), n)
    tag = AS.tag(key, nonce, g, aad(cover), ct, n)
    frame = AS.nonce12(g, nonce) + tag
    assert len(frame) * 8 == FRAME_BITS
    return np.concatenate([_bits(frame, FRAME_BITS), _bits(AS.row_bytes(ct, n), n)]), tag


def _set_flag(stego: np.ndarray) -> None:
    H, W = stego.shape
    flat = stego.ravel()   # a view: stego is contiguous
    flat[H * W - 1 - FLAG_SIDE_BIT] |= 1


def embed(cover: np.ndarray, bits, T: int, key: bytes, nonce: bytes, g: int = 0, maxval: Optional[int] = None,
          max_entries: int = 256) -> Tuple[np.ndarray, Tuple[int, ...], Dict, bytes]:
    """(stego, info, plan, tag); info[1] is the header's n_user, frame included.  A refused slice is
    its cover, with BS's refusal info."""
    user, tag = seal(cover, bits, key, nonce, g)
    stego, info, p = BS.embed(cover, user, T, maxval, checksum=False, max_entries=max_entries)
    if info[0] == 0:
        _set_flag(stego)
    return stego, info, p, tag


def choose(cover: np.ndarray, n_ct: int, tmax: int, maxval: Optional[int] = None, max_entries: int = 256) -> int:
    for T in range(1, int(tmax) + 1):
        if BS.plan(cover, FRAME_BITS + int(n_ct), T, maxval, max_entries)["status"] == 0:
            return T
    return 0


def embed_auto(cover: np.ndarray, bits, tmax: int, key: bytes, nonce: bytes, g: int = 0, maxval: Optional[int] = None,
               max_entries: int = 256):
    """(stego, info, T, tag): embed at choose()'s T, or the refusal of tmax with T = 0."""
    T = choose(cover, np.asarray(bits).size, tmax, maxval, max_entries)
    stego, info, _p, tag = embed(cover, bits, T if T else int(tmax), key, nonce, g, maxval, max_entries)
    return stego, info, T, tag


def capacity(cover: np.ndarray, T: int, maxval: Optional[int] = None, max_entries: int = 256) -> int:
    c = BS.capacity(cover, T, maxval, max_entries) - FRAME_BITS
    return c if c >= 0 else -1


def check_flags(stego: np.ndarray) -> Tuple[int, int]:
    """(flags, n_user) of a slice with a header; ValueError unless flags == 2 and n_user >= 224."""
    H, W = stego.shape
    if H * W < BS.HDR_BITS:
        raise ValueError("the slice cannot hold a header")
    w = [int(v) for v in BS.read_words(stego, 0, BS.HDR_WORDS)]
    if w[0] != BS.MAGIC:
        raise ValueError(f"magic = {w[0]:#010x} (no blind MED-PEE header)")
    flags, n_user = (w[1] >> 8) & 0xFF, w[2]
    if flags != FLAG_KEYED:
        raise ValueError(f"flags = {flags:#x} (a keyed slice has exactly {FLAG_KEYED:#x})")
    if n_user < FRAME_BITS:
        raise ValueError(f"n_user = {n_user} (a keyed slice holds the {FRAME_BITS} frame bits)")
    return flags, n_user


def unframe(user: np.ndarray) -> Tuple[int, bytes, bytes, list, int]:
    """(g, nonce, tag, CT row, n_ct) of a slice's user bits."""
    frame = np.packbits(user[:FRAME_BITS], bitorder="little").tobytes()
    ct_bits = user[FRAME_BITS:]
    return int.from_bytes(frame[:4], "little"), frame[4:12], frame[12:28], _row(ct_bits), int(ct_bits.size)


def decode(stego: np.ndarray, key: bytes, verify: bool = True) -> Tuple[np.ndarray, np.ndarray, Dict]:
    """(payload bits, cover, header).  ValueError without a keyed header; TagMismatch when the tag of
    (restored cover, CT) is not the frame's (verify=False: decrypt regardless)."""
    check_flags(stego)
    plain = stego.copy()   # BS's rules with the flag admitted: the same slice with the flag bit clear
    H, W = plain.shape
    plain.ravel()[H * W - 1 - FLAG_SIDE_BIT] &= ~np.asarray(1, plain.dtype)
    user, cover, h = BS.decode(plain, verify=False)
    g, nonce, tag, ct, n_ct = unframe(user)
    h = dict(h, flags=FLAG_KEYED, g=g, nonce=nonce, tag=tag)
    if verify:
        ok, pt = AS.release(key, nonce, g, AS.tag(key, nonce, g, aad(cover), ct, n_ct), tag, ct, n_ct)
        if not ok:
            raise TagMismatch("the tag of the restored cover and the ciphertext is not the frame's")
    else:
        pt = AS.crypt_row(key, nonce, g, ct, n_ct)
    return _bits(AS.row_bytes(pt, n_ct), n_ct), cover, h

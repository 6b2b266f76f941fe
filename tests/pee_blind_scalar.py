"""Scalar restatement of blind MED-PEE: plain Python loops and ints, one candidate and one bit at a
time, written from the header of tests/pee_blind_spec.py (no numpy, no import of the vectorised
specs or the oracle, no helper shared with them; the CRC is zlib's).  Test infrastructure: it
cross-checks the vectorised spec and generates the known-answer vectors
(tests/golden/make_pee_blind_golden.py).  Images are lists of rows of ints.
"""
from __future__ import annotations

import zlib

MAGIC = 0x4D504231
PAD = 0xFFFFFFFF


def _pred(a: int, b: int, c: int) -> int:
    hi, lo = (a, b) if a >= b else (b, a)
    if c >= hi:
        return lo
    if c <= lo:
        return hi
    return a + b - c


def _kind(v: int, p: int, T: int, maxval: int):
    """("expand" | "up" | "down", fits)"""
    e = v - p
    if -T <= e < T:
        return "expand", p + 2 * e >= 0 and p + 2 * e + 1 <= maxval
    if e >= T:
        return "up", v + T <= maxval
    return "down", v - T >= 0


def crc(img, nbytes: int) -> int:
    raw = bytearray()
    for row in img:
        for v in row:
            raw += int(v).to_bytes(nbytes, "little")
    return zlib.crc32(bytes(raw)) & 0xFFFFFFFF


def plan(img, n_user: int, T: int, maxval: int, max_entries: int = 256):
    """(status, E, n_side, i_star, first reserved pixel row)"""
    H, W = len(img), len(img[0])
    hc = H // 2
    cap = uns = 0
    for i in range(hc):
        y = 2 * i + 1
        for x in range(1, W - W % 2, 2):
            _k, fits = _kind(img[y][x], _pred(img[y][x - 1], img[y - 1][x], img[y - 1][x - 1]), T, maxval)
            if not fits:
                uns += 1
            elif _k == "expand":
                cap += 1
        if cap >= n_user + 192 + 32 * uns:
            n_side = 192 + 32 * uns
            r = (n_side + 2 * W - 1) // (2 * W)
            if i >= hc - r:
                return 1, uns, 0, i, 0
            if uns > max_entries:
                return 2, uns, 0, i, 0
            return 0, uns, n_side, i, 2 * (hc - r)
    return 1, 0, 0, -1, 0


def capacity(img, T: int, maxval: int, max_entries: int = 256) -> int:
    """The largest n_user that plan() accepts, by trying them in turn (-1: none).  A payload that
    fits leaves room for every shorter one: its row comes no later."""
    n = 0
    while plan(img, n, T, maxval, max_entries)[0] == 0:
        n += 1
    return n - 1


def _set_lsb(img, W, flat, bit):
    y, x = divmod(flat, W)
    img[y][x] = (img[y][x] & ~1) | bit


def embed(img, bits, T: int, maxval: int, nbytes: int, checksum: bool = False, max_entries: int = 256):
    """(stego, info): info = (status, n_user, E, n_side, end, region row)."""
    H, W = len(img), len(img[0])
    status, E, n_side, _i, y0 = plan(img, len(bits), T, maxval, max_entries)
    out = [list(r) for r in img]
    if status:
        return out, (status, len(bits), E, 0, -1, 0)
    payload = [img[(H * W - 1 - i) // W][(H * W - 1 - i) % W] & 1 for i in range(n_side)] + [int(b) for b in bits]
    cur, end, entries, k = 0, -1, [], 0
    for y in range(1, y0, 2):
        for x in range(1, W - W % 2, 2):
            if cur == len(payload):
                break
            v, p = img[y][x], _pred(img[y][x - 1], img[y - 1][x], img[y - 1][x - 1])
            move, fits = _kind(v, p, T, maxval)
            idx = (y // 2) * (W // 2) + x // 2
            end = idx
            if not fits:
                entries.append(idx)
            elif move == "expand":
                out[y][x] = p + 2 * (v - p) + payload[cur]
                cur += 1
            elif move == "up":
                out[y][x] = v + T
            else:
                out[y][x] = v - T
        if cur == len(payload):
            break
    assert cur == len(payload) and len(entries) <= E
    words = [MAGIC, T | ((1 if checksum else 0) << 8) | (maxval << 16), len(bits), E, end & 0xFFFFFFFF,
             crc(img, nbytes) if checksum else 0] + entries + [PAD] * (E - len(entries))
    for k, w in enumerate(words):
        for j in range(32):
            _set_lsb(out, W, H * W - 1 - (32 * k + j), (w >> j) & 1)
    return out, (0, len(bits), E, n_side, end, y0)


def _word(img, k: int) -> int:
    H, W = len(img), len(img[0])
    w = 0
    for j in range(32):
        flat = H * W - 1 - (32 * k + j)
        w |= (img[flat // W][flat % W] & 1) << j
    return w


def decode(stego):
    """(user bits, cover, (T, flags, maxval, n_user, E, end, crc)); ValueError without a header."""
    H, W = len(stego), len(stego[0])
    if H * W < 192 or _word(stego, 0) != MAGIC:
        raise ValueError("no header")
    w1, n_user, E, w4, crc_word = (_word(stego, k) for k in range(1, 6))
    T, flags, maxval = w1 & 0xFF, (w1 >> 8) & 0xFF, w1 >> 16
    end = -1 if w4 == PAD else w4
    n_side = 192 + 32 * E
    r = (n_side + 2 * W - 1) // (2 * W)
    y0 = 2 * (H // 2 - r)
    if T < 1 or n_side > H * W or y0 < 0 or end >= (y0 // 2) * (W // 2):
        raise ValueError("bad header")
    skip = {_word(stego, 6 + k) for k in range(E)} - {PAD}
    out = [list(row) for row in stego]
    got = []
    for idx in range(end + 1):
        y, x = 2 * (idx // (W // 2)) + 1, 2 * (idx % (W // 2)) + 1
        if idx in skip:
            continue
        v = stego[y][x]
        p = _pred(stego[y][x - 1], stego[y - 1][x], stego[y - 1][x - 1])
        e2 = v - p
        if -2 * T <= e2 < 2 * T:
            got.append(e2 & 1)
            out[y][x] = p + (e2 >> 1)
        elif e2 >= 2 * T:
            out[y][x] = v - T
        else:
            out[y][x] = v + T
    got = got[:n_side + n_user]
    if len(got) != n_side + n_user:
        raise ValueError("short payload")
    for i in range(n_side):
        _set_lsb(out, W, H * W - 1 - i, got[i])
    return got[n_side:], out, (T, flags, maxval, n_user, E, end, crc_word)

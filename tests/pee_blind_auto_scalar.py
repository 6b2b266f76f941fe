"""Scalar restatement of blind MED-PEE with capacity control: plain Python loops and ints, one
candidate and one bit at a time, written from the header of tests/pee_blind_auto_spec.py and of
tests/pee_blind_spec.py (no numpy, no import of the specs, the oracle or the fixed-T restatement,
no helper shared with them; the CRC is zlib's).  It classifies a candidate ONCE for every T, by the
closed form the row pass of codec_blind.hip uses, so that form is checked against the spec's
per-T classification wherever the two statements are compared.  Images are lists of rows of ints.

  closed form   e = x - MED; u = e for e >= 0 and -e - 1 otherwise;
                ok = p + 2 e >= 0 and p + 2 e + 1 <= maxval; d = maxval - x for e >= 0, x otherwise.
                At T the candidate is expandable and safe iff ok and u < T, and unsafe iff
                (u < T and not ok) or (u >= T and T > d)
"""
from __future__ import annotations

import zlib

MAGIC = 0x4D504231
PAD = 0xFFFFFFFF
HDR_BITS = 192


def _median_pred(w: int, n: int, nw: int) -> int:
    return sorted((w, n, w + n - nw))[1]


def _once(img, y: int, x: int, maxval: int):
    """(p, e, u, ok, d) of the candidate at pixel (y, x)."""
    v = img[y][x]
    p = _median_pred(img[y][x - 1], img[y - 1][x], img[y - 1][x - 1])
    e = v - p
    u = e if e >= 0 else -e - 1
    ok = 0 <= p + 2 * e and p + 2 * e + 1 <= maxval
    d = maxval - v if e >= 0 else v
    return p, e, u, ok, d


def table(img, tmax: int, maxval: int):
    """[T - 1][i] = (expandable and safe, unsafe) of candidate row i at T, one visit per candidate."""
    H, W = len(img), len(img[0])
    out = [[[0, 0] for _ in range(H // 2)] for _ in range(tmax)]
    for i in range(H // 2):
        for j in range(W // 2):
            _p, _e, u, ok, d = _once(img, 2 * i + 1, 2 * j + 1, maxval)
            for T in range(1, tmax + 1):
                if u < T:
                    out[T - 1][i][0 if ok else 1] += 1
                elif T > d:
                    out[T - 1][i][1] += 1
    return out


def plan_rows(rows, n_user: int, H: int, W: int, max_entries: int):
    """(status, E, n_side, i_star, first reserved pixel row, capacity) from one T's row counts."""
    hc = H // 2
    cap = uns = 0
    found = None
    best = -1
    for i in range(hc):
        cap += rows[i][0]
        uns += rows[i][1]
        n_side = HDR_BITS + 32 * uns
        r = -(-n_side // (2 * W))
        if found is None and cap >= n_user + n_side:
            found = (i, uns, n_side, r)
        if i < hc - r and uns <= max_entries:
            best = max(best, cap - n_side)
    if found is None:
        return 1, 0, 0, -1, 0, best
    i, E, n_side, r = found
    if i >= hc - r:
        return 1, E, 0, i, 0, best
    if E > max_entries:
        return 2, E, 0, i, 0, best
    return 0, E, n_side, i, 2 * (hc - r), best


def choose(img, n_user: int, tmax: int, maxval: int, max_entries: int = 256):
    """(T* or 0, the plan at T* (at tmax when refused), the capacity at every T)."""
    if not 1 <= tmax <= 16:
        raise ValueError("tmax in 1..16")
    H, W = len(img), len(img[0])
    tab = table(img, tmax, maxval)
    plans = [plan_rows(tab[T - 1], n_user, H, W, max_entries) for T in range(1, tmax + 1)]
    curve = [p[5] for p in plans]
    for T in range(1, tmax + 1):
        if plans[T - 1][0] == 0:
            return T, plans[T - 1], curve
    return 0, plans[-1], curve


def _crc(img, nbytes: int) -> int:
    raw = bytearray()
    for row in img:
        for v in row:
            raw += int(v).to_bytes(nbytes, "little")
    return zlib.crc32(bytes(raw)) & 0xFFFFFFFF


def embed(img, bits, tmax: int, maxval: int, nbytes: int, checksum: bool = False, max_entries: int = 256):
    """(stego, info, T*): info = (status, n_user, E, n_side, end, region row)."""
    H, W = len(img), len(img[0])
    T, (status, E, n_side, _i, y0, _cap), _curve = choose(img, len(bits), tmax, maxval, max_entries)
    out = [list(r) for r in img]
    if T == 0:
        return out, (status, len(bits), E, 0, -1, 0), 0
    stream = [img[(H * W - 1 - k) // W][(H * W - 1 - k) % W] & 1 for k in range(n_side)] + [int(b) for b in bits]
    pos, end, entries = 0, -1, []
    for idx in range((y0 // 2) * (W // 2)):
        if pos == len(stream):
            break
        y, x = 2 * (idx // (W // 2)) + 1, 2 * (idx % (W // 2)) + 1
        p, e, u, ok, d = _once(img, y, x, maxval)
        end = idx
        if u < T:
            if ok:
                out[y][x] = p + 2 * e + stream[pos]
                pos += 1
            else:
                entries.append(idx)
        elif T > d:
            entries.append(idx)
        else:
            out[y][x] = img[y][x] + (T if e >= 0 else -T)
    assert pos == len(stream) and len(entries) <= E
    words = [MAGIC, T | (int(checksum) << 8) | (maxval << 16), len(bits), E, end & 0xFFFFFFFF,
             _crc(img, nbytes) if checksum else 0] + entries + [PAD] * (E - len(entries))
    for k, w in enumerate(words):
        for j in range(32):
            flat = H * W - 1 - (32 * k + j)
            out[flat // W][flat % W] = (out[flat // W][flat % W] & ~1) | ((w >> j) & 1)
    return out, (0, len(bits), E, n_side, end, y0), T


def header_words(stego, count: int):
    H, W = len(stego), len(stego[0])
    return [sum((stego[(H * W - 1 - (32 * k + j)) // W][(H * W - 1 - (32 * k + j)) % W] & 1) << j for j in range(32))
            for k in range(count)]

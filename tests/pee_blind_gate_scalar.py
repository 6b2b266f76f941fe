"""Scalar restatement of gated blind MED-PEE: plain Python loops and ints, one candidate and one bit
at a time, written from the header of tests/pee_blind_gate_spec.py and of tests/pee_blind_spec.py (no
numpy, no import of the specs, the oracle or the other restatements, no helper shared with them; the
CRC is zlib's).  It classifies a candidate ONCE for every (T, gate): by the closed form over T that the
row pass of codec_blind.hip uses, and by the closed form of the roughness class that
codec_blind_gate.hip uses, so both forms are checked against the spec's per-pair classification
wherever the two statements are compared.  Images are lists of rows of ints.

  closed form   e = x - MED; u = e for e >= 0 and -e - 1 otherwise;
                ok = p + 2 e >= 0 and p + 2 e + 1 <= maxval; d = maxval - x for e >= 0, x otherwise.
                At T the candidate is expandable and safe iff ok and u < T, and unsafe iff
                (u < T and not ok) or (u >= T and T > d)
  class         D = max(W, N, NW) - min(W, N, NW); j = D for D <= 4; else with x = D - 1, m the
                position of x's leading one and s the bit below it, j = 1 + 2 m + s while x < 128,
                and 15 from there on.  The candidate is active at gate index g iff j <= g
"""
from __future__ import annotations

import zlib

MAGIC = 0x4D504231
PAD = 0xFFFFFFFF
HDR_BITS = 192
LADDER = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535)
FLAG_GATED = 8


def _median_pred(w: int, n: int, nw: int) -> int:
    return sorted((w, n, w + n - nw))[1]


def rough_class(D: int) -> int:
    if D <= 4:
        return D
    x = D - 1
    if x >= 128:
        return 15
    m = x.bit_length() - 1
    return 1 + 2 * m + ((x >> (m - 1)) & 1)


def _once(img, y: int, x: int, maxval: int):
    """(p, e, u, ok, d, j) of the candidate at pixel (y, x)."""
    v = img[y][x]
    w, n, nw = img[y][x - 1], img[y - 1][x], img[y - 1][x - 1]
    p = _median_pred(w, n, nw)
    e = v - p
    u = e if e >= 0 else -e - 1
    ok = 0 <= p + 2 * e and p + 2 * e + 1 <= maxval
    d = maxval - v if e >= 0 else v
    return p, e, u, ok, d, rough_class(max(w, n, nw) - min(w, n, nw))


def table(img, tmax: int, maxval: int):
    """[T - 1][g][i] = [expandable and safe, unsafe] among the candidates of row i active at gate
    index g, one visit per candidate."""
    H, W = len(img), len(img[0])
    out = [[[[0, 0] for _ in range(H // 2)] for _ in range(16)] for _ in range(tmax)]
    for i in range(H // 2):
        for c in range(W // 2):
            _p, _e, u, ok, d, j = _once(img, 2 * i + 1, 2 * c + 1, maxval)
            for T in range(1, tmax + 1):
                if u < T:
                    out[T - 1][j][i][0 if ok else 1] += 1   # into its own class first
                elif T > d:
                    out[T - 1][j][i][1] += 1
        for T in range(tmax):   # the row is complete: active at g = every class up to g
            for g in range(1, 16):
                out[T][g][i][0] += out[T][g - 1][i][0]
                out[T][g][i][1] += out[T][g - 1][i][1]
    return out


def plan_rows(rows, n_user: int, H: int, W: int, max_entries: int):
    """(status, E, n_side, i_star, first reserved pixel row, capacity) from one pair's row counts."""
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


def choose(img, n_user: int, tmax: int, maxval: int, max_entries: int = 256, t_fixed: int = 0, j_fixed: int = -1):
    """(T* or 0, j* or -1, the plan there (at the last pair considered when refused), the capacity at
    every pair [tmax][16])."""
    if not 1 <= tmax <= 16 or not 0 <= t_fixed <= tmax or not -1 <= j_fixed <= 15:
        raise ValueError("tmax in 1..16, t_fixed in 0..tmax, j_fixed in -1..15")
    H, W = len(img), len(img[0])
    tab = table(img, tmax, maxval)
    plans = [[plan_rows(tab[T - 1][g], n_user, H, W, max_entries) for g in range(16)] for T in range(1, tmax + 1)]
    curve = [[p[5] for p in row] for row in plans]
    ts = [t_fixed] if t_fixed else list(range(1, tmax + 1))
    gs = [j_fixed] if j_fixed >= 0 else list(range(16))
    for T in ts:
        for g in gs:
            if plans[T - 1][g][0] == 0:
                return T, g, plans[T - 1][g], curve
    return 0, -1, plans[ts[-1] - 1][gs[-1]], curve


def _crc(img, nbytes: int) -> int:
    raw = bytearray()
    for row in img:
        for v in row:
            raw += int(v).to_bytes(nbytes, "little")
    return zlib.crc32(bytes(raw)) & 0xFFFFFFFF


def embed(img, bits, tmax: int, maxval: int, nbytes: int, checksum: bool = False, max_entries: int = 256,
          t_fixed: int = 0, j_fixed: int = -1):
    """(stego, info, T*, G*): info = (status, n_user, E, n_side, end, region row); refused: 0 and -1."""
    H, W = len(img), len(img[0])
    T, g, (status, E, n_side, _i, y0, _cap), _curve = choose(img, len(bits), tmax, maxval, max_entries, t_fixed, j_fixed)
    out = [list(r) for r in img]
    if T == 0:
        return out, (status, len(bits), E, 0, -1, 0), 0, -1
    stream = [img[(H * W - 1 - k) // W][(H * W - 1 - k) % W] & 1 for k in range(n_side)] + [int(b) for b in bits]
    pos, end, entries = 0, -1, []
    for idx in range((y0 // 2) * (W // 2)):
        if pos == len(stream):
            break
        y, x = 2 * (idx // (W // 2)) + 1, 2 * (idx % (W // 2)) + 1
        p, e, u, ok, d, j = _once(img, y, x, maxval)
        end = idx
        if j > g:
            continue   # inactive: not modified, no entry, no bit
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
    flags = int(checksum) | FLAG_GATED | (g << 4)
    words = [MAGIC, T | (flags << 8) | (maxval << 16), len(bits), E, end & 0xFFFFFFFF,
             _crc(img, nbytes) if checksum else 0] + entries + [PAD] * (E - len(entries))
    for k, w in enumerate(words):
        for b in range(32):
            flat = H * W - 1 - (32 * k + b)
            out[flat // W][flat % W] = (out[flat // W][flat % W] & ~1) | ((w >> b) & 1)
    return out, (0, len(bits), E, n_side, end, y0), T, LADDER[g]


def _word(stego, k: int) -> int:
    H, W = len(stego), len(stego[0])
    return sum((stego[(H * W - 1 - (32 * k + b)) // W][(H * W - 1 - (32 * k + b)) % W] & 1) << b for b in range(32))


def decode(stego):
    """(user bits, cover) of a gated or an ungated slice with a valid header (no checks: the spec's
    decoder refuses, this one only undoes)."""
    H, W = len(stego), len(stego[0])
    wc = W // 2
    w1, n_user, E, end = _word(stego, 1), _word(stego, 2), _word(stego, 3), _word(stego, 4)
    T, flags = w1 & 0xFF, (w1 >> 8) & 0xFF
    g = (flags >> 4) & 15 if flags & FLAG_GATED else 15
    end = -1 if end == PAD else end
    n_side = HDR_BITS + 32 * E
    unsafe = {v for v in (_word(stego, 6 + k) for k in range(E)) if v != PAD}
    cover = [list(r) for r in stego]
    got = []
    for idx in range(end + 1):
        y, x = 2 * (idx // wc) + 1, 2 * (idx % wc) + 1
        w, n, nw = stego[y][x - 1], stego[y - 1][x], stego[y - 1][x - 1]
        if idx in unsafe or rough_class(max(w, n, nw) - min(w, n, nw)) > g:
            continue
        p = _median_pred(w, n, nw)
        e2 = stego[y][x] - p
        if -2 * T <= e2 < 2 * T:
            got.append(e2 & 1)
            cover[y][x] = p + (e2 >> 1)
        else:
            cover[y][x] = stego[y][x] - T if e2 >= 2 * T else stego[y][x] + T
    got = got[:n_side + n_user]
    for k in range(n_side):
        flat = H * W - 1 - k
        cover[flat // W][flat % W] = (cover[flat // W][flat % W] & ~1) | got[k]
    return got[n_side:], cover

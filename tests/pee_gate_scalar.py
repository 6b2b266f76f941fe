"""Scalar restatement of smoothness-gated MED-PEE: plain Python loops and ints, one candidate
at a time, written from the specification in tests/pee_gate_spec.py's header (no numpy, no
import of the vectorised spec or the oracle).  Test infrastructure: it cross-checks the
vectorised spec and generates the known-answer vectors (tests/golden/make_pee_gate_golden.py),
as tests/pee_scalar.py does for the ungated scheme.
"""
from __future__ import annotations

GATES = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535)


def _med(a: int, b: int, c: int) -> int:
    if c >= max(a, b):
        return min(a, b)
    if c <= min(a, b):
        return max(a, b)
    return a + b - c


def _cands(img):
    """(y, x, value, prediction, roughness) of every (odd, odd) candidate, row by row."""
    out = []
    for y in range(1, len(img), 2):
        for x in range(1, len(img[0]), 2):
            a, b, c = img[y][x - 1], img[y - 1][x], img[y - 1][x - 1]
            out.append((y, x, img[y][x], _med(a, b, c), max(a, b, c) - min(a, b, c)))
    return out


def embed(img, bits, T: int, G: int, maxval: int):
    """embed() one candidate at a time on lists of ints."""
    cands = _cands(img)
    kinds = []   # None: inactive; else (kind, safe)
    for _y, _x, v, p, d in cands:
        if d > G:
            kinds.append(None)
            continue
        e = v - p
        if -T <= e < T:
            kinds.append(("e", 0 <= p + 2 * e and p + 2 * e + 1 <= maxval))
        elif e >= T:
            kinds.append(("r", v + T <= maxval))
        else:
            kinds.append(("l", v - T >= 0))
    capacity = sum(1 for kd in kinds if kd == ("e", True))
    L, status = len(bits), 0
    if capacity < L:
        bits, L, status, end = bits[:capacity], capacity, 1, len(cands) - 1
    else:
        end, seen = -1, 0
        for idx, kd in enumerate(kinds):
            if L and kd == ("e", True):
                seen += 1
                if seen == L:
                    end = idx
                    break
    out = [list(r) for r in img]
    lm, cur = [], 0
    for idx, ((y, x, v, p, _d), kd) in enumerate(zip(cands, kinds)):
        if idx > end:
            break
        lm.append(kd is not None and not kd[1])
        if kd is None or not kd[1]:
            continue
        if kd[0] == "e":
            out[y][x] = p + 2 * (v - p) + int(bits[cur])
            cur += 1
        elif kd[0] == "r":
            out[y][x] = v + T
        else:
            out[y][x] = v - T
    return out, {"T": T, "G": G, "L": L, "end": end, "maxval": maxval, "lm": lm, "capacity": capacity,
                 "status": status, "lm_count": sum(lm)}


def extract(stego, side):
    T, G, end, L = side["T"], side["G"], side["end"], side["L"]
    out = [list(r) for r in stego]
    bits = []
    for idx, (y, x, v, p, d) in enumerate(_cands(stego)):
        if idx > end:
            break
        if side["lm"][idx] or d > G:
            continue
        e2 = v - p
        if -2 * T <= e2 < 2 * T:
            bits.append(e2 & 1)
            out[y][x] = p + (e2 >> 1)
        elif e2 >= 2 * T:
            out[y][x] = v - T
        else:
            out[y][x] = v + T
    return bits[:L], out


def table(img, tmax: int, maxval: int):
    n = [0] * 16
    hs = [[0] * 16 for _ in range(tmax)]
    for _y, _x, v, p, d in _cands(img):
        j = 0
        while d > GATES[j]:
            j += 1
        n[j] += 1
        e = v - p
        u = e if e >= 0 else -e - 1
        if u < tmax and 0 <= p + 2 * e and p + 2 * e + 1 <= maxval:
            hs[u][j] += 1
    return n, hs


def select(n, hs, L: int, t_fixed: int = 0):
    """select() with running sums, the way the device tail computes it."""
    tmax = len(hs)
    kc, sc = [0] * 16, [0] * 16
    best = None
    first = None
    last = (t_fixed or tmax, 15, 0)
    for T in range(1, tmax + 1):
        u = T - 1
        for g in range(16):
            kc[g] += hs[u][g]
            sc[g] += hs[u][g] * (u * u + (u + 1) * (u + 1))
        if t_fixed and T != t_fixed:
            continue
        K = S = N = 0
        for j in range(16):
            K += kc[j]
            S += sc[j]
            N += n[j]
            if j == 0 and first is None:
                first = (T, 0, K)
            A = 2 * T * T * (N - K) + S
            if L and K >= L and (best is None or A * best[1] < best[0] * K):
                best = (A, K, T, j)
        last = (T, 15, K)
    if L == 0:
        return first
    return (best[2], best[3], best[1]) if best else last

"""Scalar restatement of ROI-protected MED-PEE: plain Python loops and ints, one candidate at a
time, written from the header of tests/pee_roi_spec.py (no numpy, no import of the vectorised
specs or the oracle, no helper shared with them).  Test infrastructure: it cross-checks the
vectorised spec and generates the known-answer vectors (tests/golden/make_pee_roi_golden.py).
"""
from __future__ import annotations

GATES = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535)


def _pred(a: int, b: int, c: int) -> int:
    hi, lo = (a, b) if a >= b else (b, a)
    if c >= hi:
        return lo
    if c <= lo:
        return hi
    return a + b - c


def normalize(rect):
    y0, x0, y1, x1 = rect
    return (0, 0, 0, 0) if y0 == y1 or x0 == x1 else (y0, x0, y1, x1)


def _walk(img, rect, G):
    """Per candidate, in row-major order: (y, x, value, prediction, counts) -- counts is False for
    a candidate inside the rectangle or rougher than the gate."""
    y0, x0, y1, x1 = normalize(rect)
    out = []
    for y in range(1, len(img), 2):
        for x in range(1, len(img[0]), 2):
            a, b, c = img[y][x - 1], img[y - 1][x], img[y - 1][x - 1]
            inside = y0 <= y < y1 and x0 <= x < x1
            rough = max(a, b, c) - min(a, b, c)
            out.append((y, x, img[y][x], _pred(a, b, c), (not inside) and rough <= G))
    return out


def embed(img, bits, T: int, G: int, rect, maxval: int):
    cands = _walk(img, rect, G)
    plan = []   # per candidate: "skip", or (move, fits): move in "expand", "up", "down"
    for _y, _x, v, p, counts in cands:
        if not counts:
            plan.append("skip")
            continue
        e = v - p
        if -T <= e < T:
            plan.append(("expand", p + 2 * e >= 0 and p + 2 * e + 1 <= maxval))
        elif e >= T:
            plan.append(("up", v + T <= maxval))
        else:
            plan.append(("down", v - T >= 0))
    capacity = sum(1 for s in plan if s == ("expand", True))
    L, status, end = len(bits), 0, -1
    if capacity < L:
        L, status, end = capacity, 1, len(cands) - 1
    elif L:
        seen = 0
        for idx, s in enumerate(plan):
            if s == ("expand", True):
                seen += 1
                if seen == L:
                    end = idx
                    break
    out = [list(r) for r in img]
    lm, cur = [], 0
    for idx in range(end + 1):
        y, x, v, p, _counts = cands[idx]
        s = plan[idx]
        if s == "skip":
            lm.append(False)
            continue
        lm.append(not s[1])
        if not s[1]:
            continue
        if s[0] == "expand":
            out[y][x] = p + 2 * (v - p) + int(bits[cur])
            cur += 1
        elif s[0] == "up":
            out[y][x] = v + T
        else:
            out[y][x] = v - T
    y0, x0, y1, x1 = normalize(rect)
    return out, {"T": T, "G": G, "L": L, "end": end, "maxval": maxval, "lm": lm, "capacity": capacity,
                 "status": status, "lm_count": sum(lm), "roi": (y0, x0, y1, x1),
                 "reserved": ((y0 << 16) | x0, G + 1, (y1 << 16) | x1)}


def extract(stego, side):
    T, end, L = side["T"], side["end"], side["L"]
    out = [list(r) for r in stego]
    bits = []
    for idx, (y, x, v, p, counts) in enumerate(_walk(stego, side["roi"], side["G"])):
        if idx > end:
            break
        if side["lm"][idx] or not counts:
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


def table(img, tmax: int, rect, maxval: int):
    y0, x0, y1, x1 = normalize(rect)
    n = [0] * 16
    hs = [[0] * 16 for _ in range(tmax)]
    for y, x, v, p, _counts in _walk(img, rect, 65535):
        if y0 <= y < y1 and x0 <= x < x1:
            continue
        a, b, c = img[y][x - 1], img[y - 1][x], img[y - 1][x - 1]
        d = max(a, b, c) - min(a, b, c)
        j = next(i for i, g in enumerate(GATES) if d <= g)
        n[j] += 1
        e = v - p
        u = e if e >= 0 else -e - 1
        if u < tmax and p + 2 * e >= 0 and p + 2 * e + 1 <= maxval:
            hs[u][j] += 1
    return n, hs


def select(n, hs, L: int, t_fixed: int = 0):
    """(T, j, K) by exhaustive search over the pairs, the rule as the header of
    include/codec_tcc_gate.h states it."""
    tmax = len(hs)
    ts = [t_fixed] if t_fixed else list(range(1, tmax + 1))

    def K(T, j):
        return sum(hs[u][g] for u in range(T) for g in range(j + 1))

    if L == 0:
        return ts[0], 0, K(ts[0], 0)
    best = None
    for T in ts:
        for j in range(16):
            k = K(T, j)
            if k >= L and k > 0:
                A = 2 * T * T * (sum(n[: j + 1]) - k) + sum(hs[u][g] * (u * u + (u + 1) * (u + 1))
                                                             for u in range(T) for g in range(j + 1))
                if best is None or A * best[1] < best[0] * k:
                    best = (A, k, T, j)
    if best is None:
        return ts[-1], 15, K(ts[-1], 15)
    return best[2], best[3], best[1]

"""Specification of smoothness-gated MED-PEE (scheme 1): embed only where the MED context is
flat.  TEST INFRASTRUCTURE ONLY: the HIP kernels (codec_tcc_amd/csrc/codec_pee.hip's GATE
instantiations, codec_gate.hip) are checked bit-exact against embed() / extract() / table() /
select(), and those against the scalar restatement tests/pee_gate_scalar.py (plain Python loops
and ints, as tests/pee_scalar.py is for the ungated scheme).

All integer.  For a candidate with MED neighbours a = W, b = N, c = NW (never modified by
scheme 1, so the decoder reads the same values):
  roughness  D = max(a, b, c) - min(a, b, c)
  gate       G in 0..65535; the candidate is ACTIVE iff D <= G
  inactive   never modified, location-map bit 0, carries no bit, counts towards nothing
             (capacity, the bit cursor, lm_count, the decoder's inner-candidate counts)
  active     oracle/pee_cpu.py's scheme exactly: classify, expand / shift, the overflow map,
             the bit order, `end` = the index (over ALL candidates) of the one carrying bit
             L - 1, truncation (end = nc - 1, status 1), decode
  G = 65535  is pee_cpu.pee_embed bit for bit
  record     codec_pee_meta.reserved[1] = G + 1 (0 = ungated: every earlier record)
  ladder     GATES; a candidate's class is the first j with D <= GATES[j]
  table      n[j] = candidates of class j; hs[u][j] = those whose expansion is safe
             (capacity_curve's test) with u = (e >= 0 ? e : -e - 1) < tmax
             K(T, j) = sum_{u < T, g <= j} hs[u][g] = the capacity at (T, GATES[j])
             N(j) = sum_{g <= j} n[g]
  selection  A(T, j) = 2 T^2 (N(j) - K(T, j)) + sum_{u < T, g <= j} hs[u][g] (u^2 + (u+1)^2)
             among pairs with K >= L and K > 0 the smallest A / K (A1 K2 < A2 K1 exactly), ties
             to the smaller T, then the smaller j; L = 0: (1, 0) [(t_fixed, 0) with a fixed T];
             no feasible pair: (tmax, 15) [(t_fixed, 15)] -- the ungated truncated embedding.
             tmax <= 16 and nc <= 2^26 keep every product below 2^64.
  fixed T    the same rule over that T only
  fixed G    (any G): the smallest T with K(T, G) >= L, tmax if none (a one-column table:
             class 0 = D <= G, class 15 = the rest)
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from oracle.pee_cpu import _grids, classify, med

GATES = (0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 65535)
GATE_MAX = 65535
TMAX_MAX = 16
NC_MAX = 1 << 26


def roughness(a, b, c):
    return np.maximum(np.maximum(a, b), c) - np.minimum(np.minimum(a, b), c)


def _maxval(img, maxval):
    return int(np.iinfo(img.dtype).max) if maxval is None else int(maxval)


def active_fraction(cover: np.ndarray, G: int) -> float:
    _x, a, b, c = _grids(cover)
    d = roughness(a, b, c)
    return float((d <= G).mean()) if d.size else 0.0


def embed(cover: np.ndarray, bits, T: int, G: int, maxval: Optional[int] = None) -> Tuple[np.ndarray, Dict]:
    """(stego, side): side as pee_cpu.pee_embed's (truncate=True) plus "G" and "lm_count"."""
    if cover.dtype not in (np.uint8, np.uint16) or cover.ndim != 2:
        raise ValueError("cover must be a 2-D uint8/uint16 image")
    if T < 1 or not 0 <= G <= GATE_MAX:
        raise ValueError("T >= 1 and 0 <= G <= 65535")
    maxval = _maxval(cover, maxval)
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    L = bits.size
    x, a, b, c = _grids(cover)
    p = med(a, b, c)
    e, expand, right, safe = classify(x, p, T, maxval)
    act = (roughness(a, b, c) <= G).ravel()
    es = (expand & safe).ravel() & act
    capacity = int(es.sum())
    status = 0
    if capacity < L:
        bits, L, status = bits[:capacity], capacity, 1
        end = es.size - 1
    else:
        end = int(np.flatnonzero(es)[L - 1]) if L else -1
    k = np.arange(es.size)
    proc = (k <= end) & safe.ravel() & act
    cursor = np.cumsum(es) - 1
    bit = np.zeros(es.size, np.int64)
    bit[es & proc] = bits[cursor[es & proc]]
    xf, pf, ef, rf = x.ravel(), p.ravel(), e.ravel(), right.ravel()
    new = np.where(es, pf + 2 * ef + bit, np.where(rf, xf + T, xf - T))
    out = np.where(proc, new, xf)
    stego = cover.copy()
    hc, wc = x.shape
    stego[1:1 + 2 * hc:2, 1:1 + 2 * wc:2] = out.reshape(hc, wc).astype(cover.dtype)
    lm = (~safe.ravel() & act)[: end + 1]
    return stego, {"T": T, "G": G, "L": L, "end": end, "maxval": maxval, "lm": lm, "capacity": capacity,
                   "status": status, "lm_count": int(lm.sum())}


def extract(stego: np.ndarray, side: Dict) -> Tuple[np.ndarray, np.ndarray]:
    T, G, end, L = side["T"], side["G"], side["end"], side["L"]
    x, a, b, c = _grids(stego)
    p = med(a, b, c).ravel()
    xf = x.ravel()
    e2 = xf - p
    k = np.arange(xf.size)
    lm = np.zeros(xf.size, bool)
    lm[: end + 1] = side["lm"]
    act = (k <= end) & ~lm & (roughness(a, b, c).ravel() <= G)
    inner = act & (e2 >= -2 * T) & (e2 < 2 * T)
    bits = (e2[inner] & 1).astype(np.uint8)[:L]
    rec = np.where(inner, p + (e2 >> 1), np.where(act & (e2 >= 2 * T), xf - T, np.where(act, xf + T, xf)))
    cover = stego.copy()
    hc, wc = x.shape
    cover[1:1 + 2 * hc:2, 1:1 + 2 * wc:2] = rec.reshape(hc, wc).astype(stego.dtype)
    return bits, cover


def gate_class(d):
    """The first j with d <= GATES[j] (vectorised)."""
    return np.searchsorted(np.asarray(GATES), d, side="left")


def table(cover: np.ndarray, tmax: int, maxval: Optional[int] = None, g_fixed: Optional[int] = None):
    """(n[16], hs[tmax][16]) as int64.  g_fixed: the one-column table of a gate outside the
    ladder -- class 0 = D <= g_fixed, class 15 = the rest."""
    maxval = _maxval(cover, maxval)
    x, a, b, c = _grids(cover)
    p = med(a, b, c)
    e = (x - p).ravel()
    p = p.ravel()
    d = roughness(a, b, c).ravel()
    j = gate_class(d) if g_fixed is None else np.where(d <= g_fixed, 0, 15)
    u = np.where(e >= 0, e, -e - 1)
    ok = (p + 2 * e >= 0) & (p + 2 * e + 1 <= maxval) & (u < tmax)
    n = np.bincount(j, minlength=16).astype(np.int64)
    hs = np.zeros((tmax, 16), np.int64)
    np.add.at(hs, (u[ok], j[ok]), 1)
    return n, hs


def K_table(hs) -> np.ndarray:
    """K[T - 1][j] = the capacity at (T, GATES[j])."""
    return np.cumsum(np.cumsum(np.asarray(hs, dtype=object), axis=0), axis=1)


def select(n, hs, L: int, t_fixed: int = 0) -> Tuple[int, int, int]:
    """(T, j, K): the rule on one slice's table, exact (Python ints)."""
    hs = [[int(v) for v in row] for row in np.asarray(hs)]
    n = [int(v) for v in np.asarray(n)]
    tmax = len(hs)
    K = K_table(hs)
    cost = np.array([[hs[u][g] * (u * u + (u + 1) * (u + 1)) for g in range(16)] for u in range(tmax)], dtype=object)
    S = np.cumsum(np.cumsum(cost, axis=0), axis=1)
    N = np.cumsum(np.asarray(n, dtype=object))
    ts = [t_fixed] if t_fixed else list(range(1, tmax + 1))
    if L == 0:
        return ts[0], 0, int(K[ts[0] - 1][0])
    best = None
    for T in ts:
        for j in range(16):
            k = int(K[T - 1][j])
            if k >= L and k > 0:
                A = 2 * T * T * (int(N[j]) - k) + int(S[T - 1][j])
                if best is None or A * best[1] < best[0] * k:
                    best = (A, k, T, j)
    if best is None:
        return ts[-1], 15, int(K[ts[-1] - 1][15])
    return best[2], best[3], best[1]


def select_T(hs, L: int, j: int = 0) -> Tuple[int, int]:
    """Fixed gate: (T, K) with the smallest T whose K(T, j) holds L (tmax if none)."""
    K = K_table(hs)
    for T in range(1, len(K) + 1):
        if int(K[T - 1][j]) >= L:
            return T, int(K[T - 1][j])
    return len(K), int(K[-1][j])


# ---------------------------------------------------------------- the tests' helpers
def payload_bits(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(7000 + seed).integers(0, 2, int(n)).astype(np.uint8)


def psnr(a: np.ndarray, b: np.ndarray, peak: int) -> float:
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)

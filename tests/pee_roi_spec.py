"""Specification of ROI-protected MED-PEE (scheme 1): a per-slice rectangle that the embedding
never modifies.  TEST INFRASTRUCTURE ONLY: the HIP kernels (the _roi kernels of
codec_tcc_amd/csrc/codec_pee.hip and codec_gate.hip) are checked bit-exact against embed() /
extract() / table() / select(), and those against the scalar restatement tests/pee_roi_scalar.py.

  rectangle  (y0, x0, y1, x1), half-open, 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W; one with
             y0 == y1 or x0 == x1 is empty and normalises to (0, 0, 0, 0) = no ROI
  protected  candidate (i, j) sits at pixel (2i + 1, 2j + 1); it is protected iff
             y0 <= 2i + 1 < y1 and x0 <= 2j + 1 < x1
  active     not protected and roughness D <= G (tests/pee_gate_spec.py; G = 65535 = no gate)
  inactive   as in pee_gate_spec: never modified, map bit 0, carries no bit, counts nowhere;
             `end` still indexes ALL candidates; truncation: end = nc - 1, status 1
  context    protected pixels still serve as MED neighbours of candidates outside; neither side
             modifies them, so the decoder predicts the same values
  record     reserved[0] = y0 << 16 | x0, reserved[2] = y1 << 16 | x1 (unsigned bit patterns;
             reserved[2] == 0: no ROI), reserved[1] = G + 1 always (65536 without a gate)
  table      protected candidates fall into no class: absent from n[] and hs[][]; select() and
             select_T() of pee_gate_spec then apply unchanged
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from oracle.pee_cpu import _grids, classify, med

try:   # with tests/ on the path (the suite, the golden generator) or as tests.pee_roi_spec
    import pee_gate_spec as GS
except ImportError:   # pragma: no cover
    from tests import pee_gate_spec as GS

GATE_MAX = GS.GATE_MAX
ROI_MAX_DIM = 65535
select, select_T, K_table, payload_bits = GS.select, GS.select_T, GS.K_table, GS.payload_bits


def normalize(rect, H: int, W: int) -> Tuple[int, int, int, int]:
    if rect is None:
        return 0, 0, 0, 0
    y0, x0, y1, x1 = (int(v) for v in rect)
    if not (0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W):
        raise ValueError(f"rectangle {(y0, x0, y1, x1)} outside a {H} x {W} slice")
    if H > ROI_MAX_DIM or W > ROI_MAX_DIM:
        raise ValueError("ROI calls take H, W <= 65535")
    return (0, 0, 0, 0) if y0 == y1 or x0 == x1 else (y0, x0, y1, x1)


def words(rect) -> Tuple[int, int]:
    """(reserved[0], reserved[2]) of a normalised rectangle, unsigned."""
    y0, x0, y1, x1 = rect
    return (y0 << 16) | x0, (y1 << 16) | x1


def protected(H: int, W: int, rect) -> np.ndarray:
    """bool [H // 2, W // 2]: the candidates inside the rectangle."""
    y0, x0, y1, x1 = normalize(rect, H, W)
    ys = 2 * np.arange(H // 2) + 1
    xs = 2 * np.arange(W // 2) + 1
    return ((ys >= y0) & (ys < y1))[:, None] & ((xs >= x0) & (xs < x1))[None, :]


def embed(cover: np.ndarray, bits, T: int, G: int, rect, maxval: Optional[int] = None) -> Tuple[np.ndarray, Dict]:
    """(stego, side): pee_gate_spec.embed's side plus "roi" (normalised) and "reserved" (the
    three record words, unsigned)."""
    if cover.dtype not in (np.uint8, np.uint16) or cover.ndim != 2:
        raise ValueError("cover must be a 2-D uint8/uint16 image")
    if T < 1 or not 0 <= G <= GATE_MAX:
        raise ValueError("T >= 1 and 0 <= G <= 65535")
    H, W = cover.shape
    rect = normalize(rect, H, W)
    maxval = GS._maxval(cover, maxval)
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    L = bits.size
    x, a, b, c = _grids(cover)
    p = med(a, b, c)
    e, expand, right, safe = classify(x, p, T, maxval)
    act = ((GS.roughness(a, b, c) <= G) & ~protected(H, W, rect)).ravel()
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
    w0, w2 = words(rect)
    return stego, {"T": T, "G": G, "L": L, "end": end, "maxval": maxval, "lm": lm, "capacity": capacity,
                   "status": status, "lm_count": int(lm.sum()), "roi": rect, "reserved": (w0, G + 1, w2)}


def extract(stego: np.ndarray, side: Dict) -> Tuple[np.ndarray, np.ndarray]:
    T, G, end, L = side["T"], side["G"], side["end"], side["L"]
    H, W = stego.shape
    x, a, b, c = _grids(stego)
    p = med(a, b, c).ravel()
    xf = x.ravel()
    e2 = xf - p
    k = np.arange(xf.size)
    lm = np.zeros(xf.size, bool)
    lm[: end + 1] = side["lm"]
    act = (k <= end) & ~lm & (GS.roughness(a, b, c).ravel() <= G) & ~protected(H, W, side["roi"]).ravel()
    inner = act & (e2 >= -2 * T) & (e2 < 2 * T)
    bits = (e2[inner] & 1).astype(np.uint8)[:L]
    rec = np.where(inner, p + (e2 >> 1), np.where(act & (e2 >= 2 * T), xf - T, np.where(act, xf + T, xf)))
    cover = stego.copy()
    hc, wc = x.shape
    cover[1:1 + 2 * hc:2, 1:1 + 2 * wc:2] = rec.reshape(hc, wc).astype(stego.dtype)
    return bits, cover


def table(cover: np.ndarray, tmax: int, rect, maxval: Optional[int] = None, g_fixed: Optional[int] = None):
    """(n[16], hs[tmax][16]) as int64 over the candidates outside the rectangle."""
    H, W = cover.shape
    maxval = GS._maxval(cover, maxval)
    x, a, b, c = _grids(cover)
    p = med(a, b, c)
    keep = ~protected(H, W, rect).ravel()
    e = (x - p).ravel()[keep]
    p = p.ravel()[keep]
    d = GS.roughness(a, b, c).ravel()[keep]
    j = GS.gate_class(d) if g_fixed is None else np.where(d <= g_fixed, 0, 15)
    u = np.where(e >= 0, e, -e - 1)
    ok = (p + 2 * e >= 0) & (p + 2 * e + 1 <= maxval) & (u < tmax)
    n = np.bincount(j, minlength=16).astype(np.int64)
    hs = np.zeros((tmax, 16), np.int64)
    np.add.at(hs, (u[ok], j[ok]), 1)
    return n, hs


def choose(cover: np.ndarray, L: int, tmax: int, rect, maxval: Optional[int] = None, T=None, gate=None):
    """(T, G) an embed picks under the rectangle.  T: None = "auto", else fixed; gate: None =
    "auto" (the ladder), else a fixed gate value.  At least one of them is automatic."""
    if gate is None:
        n, hs = table(cover, tmax if T is None else T, rect, maxval)
        t, j, _k = select(n, hs, L, 0 if T is None else T)
        return t, GS.GATES[j]
    _n, hs = table(cover, tmax, rect, maxval, g_fixed=gate)
    t, _k = select_T(hs, L, 0)
    return t, gate

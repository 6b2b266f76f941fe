"""Adversarial MED-PEE covers (test infrastructure; seeded, no files).

The synthetic covers of codec_tcc_amd.synth are smooth: under 0.4 % of their candidates reach
the overflow location map, all of those at pixel 0, and no prediction error exceeds +-125.  The
generators here put candidates at both range ends, errors at +-maxval, pixels above maxval and
every comparison edge of the classification into one batch:

  flat_zero    all 0: every candidate carries a bit (capacity = nc, four carriers per item)
  flat_max     all maxval: every candidate is expansion-unsafe (all-ones map, capacity 0)
  ends         every pixel independently one of {0, 1, 2} or {maxval - 2 .. maxval}: errors
               reach +-maxval, about half the candidates unsafe, on both sides
  checker      (y + x) even -> 0, odd -> maxval: e = -maxval at every candidate, all unsafe
  checker_inv  the inverse: e = +maxval everywhere
  top_band     the ct12 field rescaled to maxval and lifted so that its crest (the top 15 % of
               the pixels) saturates at maxval: small errors, unsafe candidates at the top
  above        the same field stretched over half the scale, with noise of at least T, offset so
               that its median sits on maxval: about half the pixels lie above maxval (clipped
               to the dtype's maximum, so with maxval = the dtype's maximum it is a
               half-saturated top_band)
  ladder       2x2 cells whose three MED neighbours equal v (prediction v) and whose candidate
               is clip(v + e, 0, maxval); e and v walk the lists below: every comparison of the
               classification, the 6-bit clamp edges of the resident kernel's kept error byte
               and the tmax = 16 edge, each at both range ends

cover(kind, h, w, dtype, maxval, T, seed) -> [h, w] array; batch(...) -> one slice per kind.
"""
from __future__ import annotations

import numpy as np

from codec_tcc_amd import synth

KINDS = ("flat_zero", "flat_max", "ends", "checker", "checker_inv", "top_band", "above", "ladder")


def full_scale(dtype, maxval=None) -> int:
    return int(np.iinfo(np.dtype(dtype)).max) if maxval is None else int(maxval)


def ladder_errors(T: int):
    return (-T - 1, -T, -T + 1, -1, 0, T - 2, T - 1, T, T + 1, -33, -32, -31, 29, 30, 31, 32, -17, -16, 15, 16)


def ladder_levels(T: int, mv: int):
    return (0, 1, T - 1, T, T + 1, 33, mv // 2, mv - 34, mv - T - 1, mv - T, mv - T + 1, mv - 1, mv)


def _field(h, w, seed):
    """The ct12 field (codec_tcc_amd.synth.ct12) before noise, rounding and clipping."""
    y, x = np.mgrid[0:h, 0:w]
    return (np.sin(x / 97.0 + seed) + np.cos(y / 61.0) + 2.0) / 4.0 * 4095.0 * 0.8


def cover(kind: str, h: int, w: int, dtype="uint16", maxval=None, T: int = 2, seed: int = 0) -> np.ndarray:
    dt = np.dtype(dtype)
    top = int(np.iinfo(dt).max)
    mv = full_scale(dt, maxval)
    rng = np.random.default_rng(seed)
    if kind == "flat_zero":
        img = np.zeros((h, w), np.int64)
    elif kind == "flat_max":
        img = np.full((h, w), mv, np.int64)
    elif kind == "ends":
        low = rng.integers(0, 3, (h, w))
        img = np.where(rng.integers(0, 2, (h, w)) == 1, mv - low, low)
    elif kind in ("checker", "checker_inv"):
        y, x = np.mgrid[0:h, 0:w]
        odd = ((y + x) & 1) == 1
        img = np.where(odd if kind == "checker" else ~odd, mv, 0)
    elif kind == "top_band":
        scale = mv / 4095.0
        f = (_field(h, w, seed) + rng.normal(0.0, 16.0, (h, w))) * scale
        img = np.clip(np.rint(f + (mv - np.percentile(f, 85.0))), 0, mv).astype(np.int64)
    elif kind == "above":
        # the field stretched over half the scale whatever the shape, so that a pixel's height
        # above maxval comes from the field and its error's sign from the noise
        f = _field(h, w, seed)
        f = (f - f.min()) / max(float(f.max() - f.min()), 1.0) * (0.5 * mv)
        f = f + rng.normal(0.0, max(16.0 * mv / 4095.0, float(T)), (h, w))
        img = np.clip(np.rint(f + (mv - np.median(f))), 0, top).astype(np.int64)
    elif kind == "ladder":
        E, V = ladder_errors(T), ladder_levels(T, mv)
        hc, wc = (h + 1) // 2, (w + 1) // 2
        k = np.arange(hc * wc).reshape(hc, wc) + seed
        v = np.clip(np.asarray(V, np.int64)[(k // len(E)) % len(V)], 0, mv)
        e = np.asarray(E, np.int64)[k % len(E)]
        img = np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)[:h, :w].copy()
        cand = np.clip(v + e, 0, mv)
        img[1::2, 1::2] = cand[: h // 2, : w // 2]
    else:
        raise ValueError(f"unknown cover kind {kind!r}")
    assert img.min() >= 0 and img.max() <= top
    return img.astype(dt)


def batch(h: int, w: int, dtype="uint16", maxval=None, T: int = 2, seed: int = 0) -> np.ndarray:
    """[len(KINDS), h, w]: one slice of every kind, in KINDS order."""
    return np.stack([cover(kind, h, w, dtype, maxval, T, seed + 11 * i) for i, kind in enumerate(KINDS)])


# quick self-description of a slice from the oracle alone (the CPU tests assert on these)
def describe(img: np.ndarray, T: int, maxval=None) -> dict:
    from oracle import pee_cpu as P
    mv = full_scale(img.dtype, maxval)
    x, a, b, c = P._grids(img)
    p = P.med(a, b, c)
    e, expand, right, safe = P.classify(x, p, T, mv)
    left = ~expand & ~right
    return {"nc": int(x.size), "capacity": int((expand & safe).sum()), "unsafe": int((~safe).sum()),
            "unsafe_low": int((~safe & ((left & (x - T < 0)) | (expand & (p + 2 * e < 0)))).sum()),
            "unsafe_high": int((~safe & ((right & (x + T > mv)) | (expand & (p + 2 * e + 1 > mv)))).sum()),
            "unsafe_right_shift": int((right & ~safe).sum()),
            "emin": int(e.min()) if e.size else 0, "emax": int(e.max()) if e.size else 0,
            "left_above": int((left & (x - T > mv)).sum()), "px_above": int((img.astype(np.int64) > mv).sum())}

"""Covers and cases of the blind MED-PEE tests (test infrastructure; seeded, no files).

  smooth    tests/pee_covers._field(h, w, 3) + N(0, 1.5) (default_rng(3)), rounded and clipped to
            0..4095, uint16 (uint8: the field / 16 + the same noise, clipped to 0..255)
  planted   a smooth cover with a few (odd, odd) pixels set to 0 or the maximum amid mid-grey
            W / N / NW neighbours: unsafe at any T.  Each of those neighbours is context of that one
            candidate alone, so nothing else changes class
  pad       one more planted pixel in the last column of candidate row i*, past `end`: it counts
            towards E but not towards the map, so the header ends in a padding entry

CASES: (name, h, w, dtype, T, planted pixels, n_user, E, r) -- the table of DESIGN §3k.
"""
from __future__ import annotations

import numpy as np

import pee_blind_spec as BS
from pee_covers import _field

CASES = (
    ("smooth", 64, 96, "uint16", 4, 0, 200, 0, 1),
    ("planted1", 64, 96, "uint16", 4, 1, 150, 1, 2),
    ("planted3", 64, 96, "uint16", 4, 3, 150, 3, 2),
    ("wide_t2", 16, 256, "uint16", 2, 2, 150, 2, 1),
    ("wide_t4", 16, 256, "uint16", 4, 2, 150, 2, 1),
    ("odd", 37, 53, "uint16", 4, 1, 0, 1, 3),
    ("u8", 64, 96, "uint8", 2, 2, 60, 2, 2),
)


def top(dtype) -> int:
    return 4095 if np.dtype(dtype) == np.uint16 else 255


def smooth(h: int, w: int, dtype="uint16") -> np.ndarray:
    f = _field(h, w, 3)
    if np.dtype(dtype) == np.uint8:
        f = f / 16.0
    return np.clip(np.rint(f + np.random.default_rng(3).normal(0.0, 1.5, (h, w))), 0, top(dtype)).astype(dtype)


def plant(img: np.ndarray, y: int, x: int, high: bool) -> None:
    mv = top(img.dtype)
    img[y, x - 1] = img[y - 1, x] = img[y - 1, x - 1] = (mv + 1) // 2
    img[y, x] = mv if high else 0


def planted(h: int, w: int, k: int, dtype="uint16") -> np.ndarray:
    """k planted pixels in candidate rows 0, 1, ..., alternating low and high, columns apart."""
    img = smooth(h, w, dtype)
    for q in range(k):
        plant(img, 2 * q + 1, 2 * ((5 + 7 * q) % (w // 2)) + 1, q % 2 == 1)
    return img


def with_padding(img: np.ndarray, n_user: int, T: int):
    """(cover, plan): img with one more planted pixel in the last column of the row that then is
    i*, behind `end`, or (None, None) when no row serves."""
    h, w = img.shape
    wc = w // 2
    for i in range(h // 2):
        c = img.copy()
        plant(c, 2 * i + 1, 2 * (wc - 1) + 1, False)
        bits = np.zeros(n_user, np.uint8)
        _stego, info, p = BS.embed(c, bits, T, top(c.dtype))
        if info[0] == 0 and p["i_star"] == i and info[4] < i * wc + wc - 1:
            return c, p
    return None, None


def case_cover(case) -> np.ndarray:
    _name, h, w, dtype, _T, k, _n, _E, _r = case
    return planted(h, w, k, dtype)


def payload(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(4000 + seed).integers(0, 2, n).astype(np.uint8)

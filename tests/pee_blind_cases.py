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


# ---------------------------------------------------------------------------------------------
# Shapes at which the kernels' loops run more than once (tests/test_pee_blind_shapes.py on the
# GPU, tests/test_pee_blind_host.py spec against scalar restatement).  T = 4 for uint16 (maxval
# 4095) and 2 for uint8 (maxval 255); the flat covers of "narrow" take T = 2 in both.
def scattered(h: int, w: int, dtype, cells) -> np.ndarray:
    """A smooth cover with the q-th candidate (i, j) of `cells` planted, alternately low and high."""
    img = smooth(h, w, dtype)
    for q, (i, j) in enumerate(cells):
        plant(img, 2 * i + 1, 2 * j + 1, high=(q % 2 == 1))
    return img


def flat(h: int, w: int, dtype) -> np.ndarray:
    """Mid-grey everywhere: every candidate is expandable and safe at any T."""
    return np.full((h, w), (top(dtype) + 1) // 2, dtype=dtype)


def many_cells(h: int, w: int, k: int = 300):
    """k sorted picks (default_rng(11)) among the candidates with odd row and odd column number:
    no planted cell touches another's context."""
    L = [(i, j) for i in range(1, h // 2, 2) for j in range(1, w // 2, 2)]
    return [L[q] for q in sorted(np.random.default_rng(11).choice(len(L), k, replace=False).tolist())]


TALL_CELLS = ((5, 3), (260, 5), (300, 2), (520, 7), (530, 1))     # unsafe pixels in all three chunks of 256 rows
WIDE_CELLS = ((0, 400), (2, 100), (3, 500), (4, 7))
LONG_CELLS = ((3, 9), (100, 200), (200, 17))


def _tall(cap):
    return (cap, 55 * cap // 100, 0)


def _wide(cap):
    return (cap, cap // 2, 1)


def _many(cap):
    return (cap, cap // 2, 0)


def _long(cap):
    return (cap, 20000)


def _edge(cap):
    return (cap, cap + 1) if cap >= 0 else (0,)


# (name, group, h, w, dtype, T, cells (None: the flat cover), lengths(capacity), max_entries, checksum)
SHAPE_CASES = (
    ("tall_vec_u16", "tall", 1100, 24, "uint16", 4, TALL_CELLS, _tall, 256, True),
    ("tall_vec_u8", "tall", 1100, 24, "uint8", 2, TALL_CELLS, _tall, 256, False),
    ("tall_scalar_u16", "tall", 1101, 22, "uint16", 4, TALL_CELLS, _tall, 256, False),
    ("tall_scalar_u8", "tall", 1101, 22, "uint8", 2, TALL_CELLS, _tall, 256, True),
    ("wide_vec_u16", "wide", 12, 1032, "uint16", 4, WIDE_CELLS, _wide, 256, False),
    ("wide_vec_u8", "wide", 12, 1032, "uint8", 2, WIDE_CELLS, _wide, 256, True),
    ("wide_scalar_u16", "wide", 13, 1030, "uint16", 4, WIDE_CELLS, _wide, 256, True),
    ("wide_scalar_u8", "wide", 13, 1030, "uint8", 2, WIDE_CELLS, _wide, 256, False),
    ("many_u16", "many", 300, 264, "uint16", 4, "many", _many, 65536, True),
    ("many_u8", "many", 301, 262, "uint8", 2, "many", _many, 65536, False),
    ("long_u16", "long", 512, 512, "uint16", 4, LONG_CELLS, _long, 256, True),
    ("long_u8", "long", 512, 512, "uint8", 2, LONG_CELLS, _long, 256, False),
    ("narrow_600x2", "narrow", 600, 2, "uint16", 2, None, _edge, 256, True),
    ("narrow_601x3", "narrow", 601, 3, "uint8", 2, None, _edge, 256, False),
    ("narrow_120x8", "narrow", 120, 8, "uint16", 2, None, _edge, 256, True),
    ("narrow_121x9", "narrow", 121, 9, "uint8", 2, None, _edge, 256, False),
    ("narrow_14x14", "narrow", 14, 14, "uint16", 2, None, _edge, 256, True),
    ("narrow_28x14", "narrow", 28, 14, "uint16", 2, None, _edge, 256, False),
    ("narrow_2x96", "narrow", 2, 96, "uint16", 2, None, _edge, 256, True),
)
SHAPE_CASE = {c[0]: c for c in SHAPE_CASES}
# capacity at the case's max_entries, as the spec gives it on the recipes above (the issue's figures)
SHAPE_CAPACITY = {"tall_vec_u16": 2906, "wide_vec_u16": 1914, "wide_scalar_u16": 1932, "many_u16": 1937, "long_u16": 41843,
                  "narrow_600x2": 60, "narrow_601x3": 76, "narrow_120x8": 0, "narrow_121x9": 4, "narrow_14x14": -1,
                  "narrow_28x14": -1, "narrow_2x96": -1}
# (E, r) per embedded payload length, in the order of the case's lengths: the table of DESIGN §3k
SHAPE_ER = {"tall_vec_u16": ((5, 8), (3, 6), (1, 5)), "tall_vec_u8": ((5, 8), (3, 6), (1, 5)),
            "tall_scalar_u16": ((5, 8), (3, 7), (1, 6)), "tall_scalar_u8": ((5, 8), (3, 7), (1, 6)),
            "wide_vec_u16": ((4, 1), (2, 1), (1, 1)), "wide_vec_u8": ((4, 1), (2, 1), (1, 1)),
            "wide_scalar_u16": ((4, 1), (2, 1), (1, 1)), "wide_scalar_u8": ((4, 1), (2, 1), (1, 1)),
            "many_u16": ((271, 17), (172, 11), (4, 1)), "many_u8": ((166, 11), (119, 8), (40, 3)),
            "long_u16": ((19, 1), (18, 1)), "long_u8": ((156, 6), (155, 6)),
            "narrow_600x2": ((0, 48),), "narrow_601x3": ((0, 32),), "narrow_120x8": ((0, 12),), "narrow_121x9": ((0, 11),),
            "narrow_14x14": (), "narrow_28x14": (), "narrow_2x96": ()}

_made = {}


def shape_case(name: str):
    """(cover, T, maxval, max_entries, checksum, lengths, capacity) of a SHAPE_CASES entry; the cover
    is built once and is read-only."""
    if name not in _made:
        _n, _g, h, w, dtype, T, cells, lengths, me, checksum = SHAPE_CASE[name]
        if cells is None:
            img = flat(h, w, dtype)
        else:
            img = scattered(h, w, dtype, many_cells(h, w) if cells == "many" else cells)
        img.setflags(write=False)
        cap = BS.capacity(img, T, top(dtype), me)
        _made[name] = (img, T, top(dtype), me, checksum, tuple(lengths(cap)), cap)
    return _made[name]

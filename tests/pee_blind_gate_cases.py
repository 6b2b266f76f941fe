"""Covers and cases of the tests of gated blind MED-PEE (test infrastructure; seeded, no files): the
builders of tests/pee_blind_cases.py and tests/pee_blind_auto_cases.py and one more cover.

  half_busy  tests/pee_covers._field(h, w, 3) (/ 16 for uint8) + N(0, 1.5) on the left half of the
             columns and N(0, 40) on the right half (default_rng(5)), rounded and clipped to 0..4095
             (0..255): the roughness classes of the two halves differ, so the gate decides which
             candidates count

CASES: (name, max_entries, ((n_user, T*, G*), ...)) at tmax = TMAX and maxval 4095 / 255 -- the table of
DESIGN §3o; T* = 0, G* = -1: refused.  tests/test_pee_blind_gate_host.py recomputes every figure from
the spec, so a case that stops exercising what it claims fails without a GPU.
"""
from __future__ import annotations

import numpy as np

import pee_blind_auto_cases as AC
import pee_blind_cases as CS
from pee_covers import _field

TMAX = 8


def half_busy(h: int, w: int, dtype="uint16") -> np.ndarray:
    f = _field(h, w, 3)
    if np.dtype(dtype) == np.uint8:
        f = f / 16.0
    rng = np.random.default_rng(5)
    noise = np.concatenate([rng.normal(0.0, 1.5, (h, w // 2)), rng.normal(0.0, 40.0, (h, w - w // 2))], axis=1)
    return np.clip(np.rint(f + noise), 0, CS.top(dtype)).astype(dtype)


def planted_mix(dtype="uint16") -> np.ndarray:
    """half_busy(64, 96) with three planted pixels in flat context on the smooth half (tests/pee_blind_cases.plant:
    active at every gate) and three extreme pixels amid W / N / NW neighbours an eighth of the range
    apart on the busy half: unsafe at any T, active at no gate below 65535."""
    img = half_busy(64, 96, dtype)
    mv = CS.top(dtype)
    mid = (mv + 1) // 2
    for q in range(3):
        CS.plant(img, 2 * q + 1, 2 * ((5 + 7 * q) % 24) + 1, q % 2 == 1)
    for q in range(3):
        y, x = 2 * q + 3, 2 * (30 + 5 * q) + 1
        img[y, x - 1], img[y - 1, x], img[y - 1, x - 1] = mid, mid + mv // 8, mid - mv // 8
        img[y, x] = mv if q % 2 else 0
    return img


_BUILD = {
    "half_u16": lambda: half_busy(64, 96),
    "half_u8": lambda: half_busy(64, 96, "uint8"),
    "planted_mix": planted_mix,
    "odd": lambda: CS.planted(37, 53, 1),
    "tall_vec": lambda: CS.scattered(1100, 24, "uint16", CS.TALL_CELLS),
    "tall_scalar": lambda: CS.scattered(1101, 22, "uint16", CS.TALL_CELLS),
    "wide_vec": lambda: CS.scattered(12, 1032, "uint16", CS.WIDE_CELLS),
    "wide_scalar": lambda: CS.scattered(13, 1030, "uint16", CS.WIDE_CELLS),
    "xwide_vec_u16": lambda: CS.scattered(4, 30736, "uint16", AC.XWIDE_CELLS),
    "xwide_vec_u8": lambda: CS.scattered(4, 30736, "uint8", AC.XWIDE_CELLS),
    "xwide_scalar": lambda: CS.scattered(5, 7686, "uint16", AC.XWIDE_SCALAR_CELLS),
    "long": lambda: CS.scattered(512, 512, "uint16", CS.LONG_CELLS),
    "bright_me4": lambda: AC.bright("uint16"),
    "bright_me16": lambda: AC.bright("uint16"),
}

CASES = (
    ("half_u16", 256, ((0, 3, 12), (40, 3, 65535), (127, 5, 12), (303, 7, 16), (488, 0, -1))),
    ("half_u8", 256, ((0, 1, 3), (70, 1, 8), (276, 2, 32), (487, 4, 6), (569, 0, -1))),
    ("planted_mix", 256, ((0, 4, 48), (100, 5, 128), (300, 8, 24), (400, 0, -1))),
    ("odd", 256, ((0, 4, 12), (24, 4, 16), (100, 6, 16), (155, 0, -1))),
    ("tall_vec", 256, ((173, 1, 24), (569, 1, 32), (1498, 3, 24), (5093, 0, -1))),
    ("tall_scalar", 256, ((100, 1, 16), (552, 1, 24), (2634, 4, 32))),
    ("wide_vec", 256, ((100, 1, 8), (511, 1, 16), (1370, 3, 12), (2250, 0, -1))),
    ("wide_scalar", 256, ((91, 1, 8), (468, 1, 12), (1932, 4, 16))),
    ("xwide_vec_u16", 256, ((191, 1, 2), (4216, 1, 12), (13279, 4, 24), (15063, 0, -1))),
    ("xwide_vec_u8", 256, ((1, 1, 0), (3441, 1, 3), (13902, 4, 8))),
    ("xwide_scalar", 256, ((77, 1, 4), (843, 1, 12), (3495, 6, 24))),
    ("long", 256, ((2853, 1, 12), (20000, 2, 24))),
    ("bright_me4", 4, ((0, 0, -1), (100, 0, -1))),
    ("bright_me16", 16, ((0, 5, 12), (112, 5, 16), (571, 0, -1))),
)
CASE = {c[0]: c for c in CASES}
# planted_mix: the map entries at the chosen pairs (the three flat-context pixels) against the ungated
# plan's at the T embed_blind_auto picks (all six)
PLANTED_MIX_E = (3, 6)
# the fixed forms on the 64 x 96 cases: (name, n_user, T or None, gate or None, (T*, G*))
FIXED = (
    ("half_u16", 127, 6, None, (6, 12)),
    ("half_u16", 127, None, 65535, (5, 65535)),
    ("half_u16", 127, 5, 12, (5, 12)),
    ("half_u16", 127, 4, None, (0, -1)),
    ("half_u8", 276, None, 4, (3, 4)),
    ("half_u8", 276, 2, 8, (0, -1)),
    ("planted_mix", 100, 8, None, (8, 12)),
)

_made = {}


def cover(name: str) -> np.ndarray:
    """The case's cover, built once, read-only."""
    if name not in _made:
        img = _BUILD[name]()
        img.setflags(write=False)
        _made[name] = img
    return _made[name]


def payload(n: int, seed: int) -> np.ndarray:
    return CS.payload(n, seed)


def batch_slice(name: str, b: int):
    """(cover, bits) of slice b of the case's GPU batch: the case's lengths in turn; from the second
    turn on the cover has a dozen pixels of its lower half nudged by one, so that the slices of a
    batch differ."""
    _n, _me, lengths = CASE[name]
    img = cover(name)
    if b >= len(lengths):
        h, w = img.shape
        img = img.copy()
        rng = np.random.default_rng(90 + b)
        ys, xs = rng.integers(h // 2, max(h // 2 + 1, h - 8), 12), rng.integers(0, w, 12)
        img[ys, xs] = np.clip(img[ys, xs].astype(np.int64) + rng.integers(-1, 2, 12), 0, CS.top(img.dtype)).astype(img.dtype)
    return img, payload(lengths[b % len(lengths)][0], 10 * b + 1)

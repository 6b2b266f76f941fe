"""Covers and cases of the tests of blind MED-PEE with capacity control (test infrastructure;
seeded, no files): the builders of tests/pee_blind_cases.py and one more cover.

  bright    smooth(64, 96) with pixel rows 4..11, columns 40..55 set to
            clip(maxval - 2 + default_rng(9).integers(-1, 3), 0, maxval): candidates at the end of the
            range, whose class depends on T.  uint16 at maxval 4095: 10 unsafe candidates at T = 1,
            13 from T = 2 on

CASES: (name, max_entries, ((n_user, T*), ...)) at tmax = 8 and maxval 4095 / 255 -- the table of
DESIGN §3l; T* = 0: refused.  The host test recomputes every figure from the spec.  The xwide cases
are there for the row pass: rows long enough for a lane's later iterations and its mid-row widening.
"""
from __future__ import annotations

import numpy as np

import pee_blind_cases as CS

TMAX = 8


def bright(dtype="uint16") -> np.ndarray:
    img = CS.smooth(64, 96, dtype)
    mv = CS.top(dtype)
    img[4:12, 40:56] = np.clip(mv - 2 + np.random.default_rng(9).integers(-1, 3, (8, 16)), 0, mv).astype(img.dtype)
    return img


# one usable candidate row of 15368 (3843) candidates: 61 items (candidates) per lane of the row pass,
# so a lane runs sixteen iterations on the vector route and widens its byte counts within the row
XWIDE_CELLS = ((0, 15000), (0, 70))
XWIDE_SCALAR_CELLS = ((0, 3000), (0, 70))

_BUILD = {
    "smooth": lambda: CS.smooth(64, 96),
    "planted3": lambda: CS.planted(64, 96, 3),
    "smooth_u8": lambda: CS.smooth(64, 96, "uint8"),
    "odd": lambda: CS.planted(37, 53, 1),
    "bright_me16": lambda: bright("uint16"),
    "bright_me4": lambda: bright("uint16"),
    "bright_u8": lambda: bright("uint8"),
    "tall_vec": lambda: CS.scattered(1100, 24, "uint16", CS.TALL_CELLS),
    "tall_scalar": lambda: CS.scattered(1101, 22, "uint16", CS.TALL_CELLS),
    "wide_vec_u16": lambda: CS.scattered(12, 1032, "uint16", CS.WIDE_CELLS),
    "wide_vec_u8": lambda: CS.scattered(12, 1032, "uint8", CS.WIDE_CELLS),
    "wide_scalar": lambda: CS.scattered(13, 1030, "uint16", CS.WIDE_CELLS),
    "long": lambda: CS.scattered(512, 512, "uint16", CS.LONG_CELLS),
    "many": lambda: CS.scattered(300, 264, "uint16", CS.many_cells(300, 264)),
    "xwide_vec_u16": lambda: CS.scattered(4, 30736, "uint16", XWIDE_CELLS),
    "xwide_vec_u8": lambda: CS.scattered(4, 30736, "uint8", XWIDE_CELLS),
    "xwide_scalar": lambda: CS.scattered(5, 7686, "uint16", XWIDE_SCALAR_CELLS),
}

CASES = (
    ("smooth", 256, ((0, 2), (100, 3), (300, 4), (500, 5), (900, 7), (1200, 0))),
    ("planted3", 256, ((100, 3), (200, 4), (500, 6), (900, 8))),
    ("smooth_u8", 256, ((200, 1), (300, 2), (900, 3), (1200, 5))),
    ("odd", 256, ((0, 4), (100, 6), (200, 0))),
    ("bright_me16", 16, ((0, 5), (150, 6), (300, 7))),
    ("bright_me4", 4, ((0, 0), (150, 0), (300, 0))),
    ("bright_u8", 16, ((0, 2), (300, 3))),
    ("tall_vec", 256, ((500, 1), (700, 2))),
    ("tall_scalar", 256, ((300, 1), (700, 2), (1500, 3), (2500, 4))),
    ("wide_vec_u16", 256, ((300, 1), (700, 2), (1500, 3), (2500, 0))),
    ("wide_vec_u8", 256, ((300, 1), (700, 2), (1500, 3), (2500, 0))),
    ("wide_scalar", 256, ((300, 1), (700, 2), (1500, 3), (2500, 0))),
    ("long", 256, ((2500, 1), (20000, 2), (60000, 0))),
    ("many", 65536, ((0, 3), (100, 4))),
    ("xwide_vec_u16", 256, ((2000, 1), (5000, 2), (9000, 3), (14000, 5))),
    ("xwide_vec_u8", 256, ((2000, 1), (9000, 2), (14000, 5))),
    ("xwide_scalar", 256, ((0, 1), (2000, 3), (5000, 0))),
)
CASE = {c[0]: c for c in CASES}
# the statuses of bright_me4 over T = 1..8 at n_user = 0: the refusal reported is tmax's
BRIGHT_ME4_STATUS = (1, 1, 1, 1, 2, 2, 2, 2)
BRIGHT_UNSAFE = (10, 13, 13, 13, 13, 13, 13, 13)   # the uint16 bright cover's unsafe candidates at T = 1..8

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

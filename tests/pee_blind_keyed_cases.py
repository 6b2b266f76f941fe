"""Cases of the keyed blind MED-PEE tests (test infrastructure; the covers are tests/pee_blind_cases.py's,
seeded, no files): the table of DESIGN §3m.

CASES: (name, cover, T, E, n_ct values, keyed capacity).  `cover` names a CS.CASES entry or, for
long_u16, a CS.SHAPE_CASES one.  A length above the capacity is refused with status 1; E is that of
the embedded lengths (a tuple: one per length; None where every length is refused).
AUTO: (cover, ((n_ct, chosen T), ...)) at tmax = 8.
"""
from __future__ import annotations

import numpy as np

import pee_blind_cases as CS

KEY = bytes(range(0x40, 0x60))
NONCE = bytes.fromhex("0807060504030201")
TMAX = 8

CASES = (
    ("smooth", "smooth", 4, 0, (0, 1, 31, 32, 33, 63, 64, 65, 160, 161), 160),
    ("planted1", "planted1", 4, 1, (0, 33, 121), 121),
    ("planted3", "planted3", 4, 3, (0, 32, 55), 55),
    ("wide_t4", "wide_t4", 4, 2, (65, 279), 279),
    ("u8", "u8", 2, 2, (64, 413), 413),
    ("wide", "wide_t2", 2, None, (0,), -1),
    ("long_u16", "long_u16", 4, (18, 19), (20000, 41843 - 224), 41843 - 224),
)
CASE = {c[0]: c for c in CASES}
AUTO = (("smooth", ((0, 4), (100, 4), (300, 5), (600, 7))), ("planted3", ((100, 5), (600, 8))))

_covers = {}


def cover(name: str) -> np.ndarray:
    """The case's cover, built once, read-only."""
    src = CASE[name][1]
    if src not in _covers:
        if src in CS.SHAPE_CASE:
            img = CS.shape_case(src)[0]
        else:
            img = CS.case_cover(next(c for c in CS.CASES if c[0] == src))
            img.setflags(write=False)
        _covers[src] = img
    return _covers[src]


def index(name: str, q: int) -> int:
    """The global index of the case's q-th run: small ones, one near 2^31."""
    return (1 << 31) - 1 - q if name == "planted1" else 7 * q + len(name)


def payload(n: int, seed: int) -> np.ndarray:
    return CS.payload(n, 100 + seed)

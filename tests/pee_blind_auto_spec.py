"""Specification of blind MED-PEE with capacity control: T chosen per slice.  TEST INFRASTRUCTURE
ONLY: the kernels behind include/codec_tcc_blind_auto.h are checked bit-exact against choose() /
embed() / capacity_curve(), and those against the scalar restatement tests/pee_blind_auto_scalar.py.

  rule      per slice, with plan / embed of tests/pee_blind_spec.py: T* is the smallest T in
            1..tmax for which plan(cover, n_user, T, maxval, max_entries) has status 0, and the
            slice is embedded exactly as embed(cover, bits, T*, ...) embeds it: the same header,
            region and entries.  Nothing is assumed monotone in T (a shift by T can leave the range,
            so the unsafe counts, E, r and the status change from one T to the next)
  refusal   no T qualifies: the slice is copied through with no header, its info is that of the
            plan at T = tmax, its chosen T is 0
  capacity  curve[T - 1] = plan(cover, 0, T, ...)["capacity"]; the auto capacity is its maximum
  tmax      1..16
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

try:   # with tests/ on the path (the suite, the golden generator) or as tests.pee_blind_auto_spec
    import pee_blind_spec as BS
except ImportError:   # pragma: no cover
    from tests import pee_blind_spec as BS

TMAX = 16


def _check_tmax(tmax: int) -> None:
    if not 1 <= int(tmax) <= TMAX:
        raise ValueError(f"tmax in 1..{TMAX}")


def choose(cover: np.ndarray, n_user: int, tmax: int, maxval: Optional[int] = None, max_entries: int = 256) -> Tuple[int, Dict]:
    """(T*, plan at T*), or (0, plan at tmax) when no T in 1..tmax has status 0."""
    _check_tmax(tmax)
    p = None
    for T in range(1, int(tmax) + 1):
        p = BS.plan(cover, n_user, T, maxval, max_entries)
        if p["status"] == 0:
            return T, p
    return 0, p


def capacity_curve(cover: np.ndarray, tmax: int, maxval: Optional[int] = None, max_entries: int = 256) -> List[int]:
    _check_tmax(tmax)
    return [BS.capacity(cover, T, maxval, max_entries) for T in range(1, int(tmax) + 1)]


def capacity(cover: np.ndarray, tmax: int, maxval: Optional[int] = None, max_entries: int = 256) -> int:
    return max(capacity_curve(cover, tmax, maxval, max_entries))


def embed(cover: np.ndarray, bits, tmax: int, maxval: Optional[int] = None, checksum: bool = False,
          max_entries: int = 256) -> Tuple[np.ndarray, Tuple[int, ...], int, Dict]:
    """(stego, info, T*, plan): pee_blind_spec.embed at T*; refused (T* = 0): at tmax, which copies
    the cover through and reports (status, n_user, E, 0, -1, 0)."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    T, _p = choose(cover, bits.size, tmax, maxval, max_entries)
    stego, info, p = BS.embed(cover, bits, T if T else int(tmax), maxval, checksum, max_entries)
    assert (info[0] == 0) == (T != 0)
    return stego, info, T, p

"""Stacks and stream lengths of the blind volume tests (test infrastructure; seeded, no files, no GPU).
tests/test_pee_blind_volume_host.py checks the conditions below on the specification alone;
tests/test_pee_blind_volume.py runs the same cases on the GPU.

  stacks    pee_blind_volume_spec.stack: smooth covers of distinct seeds with slice 1 a one-pixel
            checkerboard (blind capacity -1: the non-carrier).  B = 3: the flat slots of the ROI embed,
            B = 9: its lane order.  64 x 96 takes the 8-pixel vector route, 37 x 53 the scalar one
            (and, 26 candidates a row, only tmax = 16 gives it room past the frame)
  lengths   N = 1; two thirds of S(tmax); S(tmax) (fits exactly); S(tmax) + 1 (refused, stack unchanged)
Every spec result is computed once and shared (result()).
"""
from __future__ import annotations

import functools

import numpy as np

import pee_blind_volume_spec as VS

VOLUME_ID = 0xC0DEC0DE
# name -> (h, w, dtype, maxval, tmax)
SHAPES = {"u16": (64, 96, "uint16", 4095, 8), "u8": (64, 96, "uint8", 255, 8), "odd": (37, 53, "uint16", 4095, 16)}
BATCHES = (3, 9)
POLICIES = ("even", "fill")
LENGTH_NAMES = ("one", "most", "fits", "over")


@functools.lru_cache(maxsize=None)
def stack(shape: str, B: int) -> np.ndarray:
    h, w, dtype, _mv, _tmax = SHAPES[shape]
    a = VS.stack(B, h, w, dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def curve(shape: str, B: int) -> np.ndarray:
    _h, _w, _dt, mv, tmax = SHAPES[shape]
    c = VS.curves(stack(shape, B), tmax, mv)
    c.setflags(write=False)
    return c


def lengths(shape: str, B: int) -> dict:
    S = int(VS.transform(curve(shape, B))[:, -1].sum())
    return {"one": 1, "most": max(2 * S // 3, 2), "fits": S, "over": S + 1}


def bits(shape: str, B: int, which: str) -> np.ndarray:
    return VS.stream_bits(lengths(shape, B)[which], 17 * B + LENGTH_NAMES.index(which))


@functools.lru_cache(maxsize=None)
def result(shape: str, B: int, policy: str, which: str, checksum: bool = True) -> dict:
    """pee_blind_volume_spec.embed of the case"""
    _h, _w, _dt, mv, tmax = SHAPES[shape]
    return VS.embed(stack(shape, B), bits(shape, B, which), volume_id=VOLUME_ID, policy=policy, tmax=tmax, maxval=mv,
                    checksum=checksum)


# ---- more slices than a workgroup has threads: 1100 slices of 48 x 64, every 97th a checkerboard
MANY = (1100, 48, 64)


@functools.lru_cache(maxsize=None)
def many_stack() -> np.ndarray:
    B, h, w = MANY
    out = [VS.checker(h, w) if b % 97 == 5 else VS.smooth(h, w, 900 + b) for b in range(B)]
    a = np.stack(out)
    a.setflags(write=False)
    return a


# ---- shares longer than one block of 16384 bits: two scattered 512 x 512 covers
@functools.lru_cache(maxsize=None)
def long_stack() -> np.ndarray:
    import pee_blind_cases as CS
    a = np.stack([CS.scattered(512, 512, "uint16", CS.LONG_CELLS), CS.scattered(512, 512, "uint16", ((7, 31), (150, 40)))])
    a.setflags(write=False)
    return a

#!/usr/bin/env python3
"""Known-answer vectors of ROI-protected MED-PEE -> tests/golden/pee_roi_kat.json.

Computed by the scalar restatement tests/pee_roi_scalar.py alone (not by the vectorised spec
tests/pee_roi_spec.py they then check).  Inputs are regenerated from their seeds
(codec_tcc_amd.synth + numpy default_rng), so the file holds only digests and small tables.

    python tests/golden/make_pee_roi_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from codec_tcc_amd import synth  # noqa: E402
import pee_roi_scalar as S  # noqa: E402

# (kind, h, w, seed, T, G, maxval or None, clip, payload rule, rectangle or a name)
#   "whole": the image; "end": a rectangle around the candidate that is `end` without one
CASES = [
    ("ct12", 32, 48, 1, 2, 65535, 4095, False, "half", (0, 0, 0, 0)),          # empty: the gated call
    ("ct12", 32, 48, 1, 2, 65535, 4095, False, "half", (5, 7, 5, 30)),         # empty (y0 == y1): normalises
    ("ct12", 32, 48, 1, 2, 65535, 4095, False, "half", "whole"),               # capacity 0, status 1
    ("ct12", 32, 48, 1, 2, 65535, 4095, False, "zero", "whole"),               # L = 0: end = -1, status 0
    ("ct12", 32, 48, 1, 2, 65535, 4095, False, "half", (9, 11, 10, 12)),       # one candidate
    ("ct12", 32, 48, 1, 2, 3, 4095, False, "half", (9, 11, 21, 33)),           # odd-coordinate edges
    ("ct12", 32, 48, 1, 2, 3, 4095, False, "half", (8, 10, 20, 32)),           # even-coordinate edges
    ("ct12", 33, 41, 2, 1, 65535, 4095, False, "half", (0, 0, 12, 17)),        # top-left corner, odd H and W
    ("ct12", 33, 41, 2, 1, 3, 4095, False, "half", (20, 30, 33, 41)),          # bottom-right corner
    ("ct12", 33, 41, 2, 4, 0, 4095, False, "cap", (0, 13, 33, 29)),            # full height
    ("ct12", 33, 41, 2, 4, 65535, 4095, False, "over", (11, 0, 23, 41)),       # full width, truncating payload
    ("ct12", 40, 40, 3, 2, 65535, 4095, True, "half", (5, 1, 31, 29)),         # cuts the saturated bands
    ("ct12", 40, 40, 3, 4, 3, 4095, True, "cap", (5, 1, 31, 29)),
    ("ct12", 24, 64, 4, 1, 65535, 4095, False, "half", "end"),                 # covers the unprotected run's `end`
    ("ct12", 24, 64, 4, 2, 3, 4095, False, "half", "end"),
    ("ct12", 24, 64, 4, 4, 65535, 4095, True, "over", (1, 11, 20, 29)),        # edges inside an 8-column item
    ("u8", 30, 32, 5, 2, 65535, None, True, "half", (7, 7, 23, 25)),
    ("u8", 30, 32, 5, 1, 3, None, False, "half", (0, 0, 30, 16)),              # left half
    ("u8", 31, 33, 6, 4, 0, None, True, "over", (15, 16, 31, 33)),
    ("u8", 31, 33, 6, 2, 65535, None, False, "cap", (1, 1, 2, 2)),             # candidate (0, 0) alone
    ("u8", 31, 33, 6, 2, 65535, None, False, "half", (29, 31, 30, 32)),        # the last candidate alone
    ("u16", 16, 24, 10, 4, 65535, None, False, "half", (3, 5, 11, 19)),
    ("u16", 17, 25, 11, 1, 3, None, False, "over", (0, 0, 17, 2)),             # first candidate column only
    ("u16", 17, 25, 11, 2, 0, None, False, "half", (16, 0, 17, 25)),           # last (unpaired) row: no candidate
]
TMAX = 8


def make_image(kind, h, w, seed, maxval, clip):
    img = synth.GENERATORS[kind](h, w, seed)
    if clip:   # bands of pixels at the range ends: active candidates that overflow
        top = int(np.iinfo(img.dtype).max) if maxval is None else int(maxval)
        rng = np.random.default_rng(50 + seed)
        img = img.copy()
        img[: h // 4] = rng.integers(0, 3, (h // 4, w))
        img[h // 4: h // 2] = top - rng.integers(0, 3, (h // 2 - h // 4, w))
    return img


def payload_bits(n, seed):
    return np.random.default_rng(1000 + seed).integers(0, 2, n).astype(np.uint8)


def sha(rows):
    return hashlib.sha256(np.asarray(rows, dtype=np.int64).tobytes()).hexdigest()


def rectangle(rect, rows, T, G, mv, seed):
    h, w = len(rows), len(rows[0])
    if rect == "whole":
        return (0, 0, h, w)
    if rect == "end":   # around the candidate carrying the last bit of the half-capacity payload without a rectangle
        cap = S.embed(rows, [], T, G, (0, 0, 0, 0), mv)[1]["capacity"]
        end = S.embed(rows, payload_bits(cap // 2, seed).tolist(), T, G, (0, 0, 0, 0), mv)[1]["end"]
        y, x = 2 * (end // (w // 2)) + 1, 2 * (end % (w // 2)) + 1
        return (max(0, y - 2), max(0, x - 4), min(h, y + 3), min(w, x + 5))
    return tuple(rect)


def case_record(c):
    kind, h, w, seed, T, G, maxval, clip, rule, rect = c
    img = make_image(kind, h, w, seed, maxval, clip)
    mv = int(np.iinfo(img.dtype).max) if maxval is None else maxval
    rows = img.astype(np.int64).tolist()
    name = rect if isinstance(rect, str) else None
    rect = rectangle(rect, rows, T, G, mv, seed)
    free = S.embed(rows, [], T, G, (0, 0, 0, 0), mv)[1]["capacity"]      # without the rectangle
    cap = S.embed(rows, [], T, G, rect, mv)[1]["capacity"]
    # "half" is half the capacity WITHOUT the rectangle: where the rectangle removes more, the embed truncates
    nbits = {"zero": 0, "half": free // 2, "cap": cap, "over": cap + 37}[rule]
    bits = payload_bits(nbits, seed).tolist()
    stego, side = S.embed(rows, bits, T, G, rect, mv)
    got, back = S.extract(stego, side)
    assert back == rows and got == bits[:side["L"]]
    y0, x0, y1, x1 = side["roi"]
    assert all(stego[y][x] == rows[y][x] for y in range(y0, y1) for x in range(x0, x1))
    n, hs = S.table(rows, TMAX, rect, mv)
    sel = {str(L): list(S.select(n, hs, L)) for L in (0, 1, max(1, cap // 2), cap, cap + 1, 10 ** 6)}
    return {"kind": kind, "h": h, "w": w, "seed": seed, "T": T, "G": G, "maxval": maxval, "clip": clip, "rule": rule,
            "rect": list(rect), "rect_name": name, "roi": list(side["roi"]), "reserved": list(side["reserved"]),
            "nbits": nbits, "L": side["L"], "end": side["end"], "capacity": cap, "status": side["status"],
            "lm_count": side["lm_count"], "stego_sha256": sha(stego), "lm_sha256": sha([int(v) for v in side["lm"]]),
            "n": n, "hs": hs, "tmax": TMAX, "select": sel}


def build():
    return {"cases": [case_record(c) for c in CASES]}


if __name__ == "__main__":
    out = build()
    path = os.path.join(HERE, "pee_roi_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(out["cases"]), "cases")

#!/usr/bin/env python3
"""Known-answer vectors of smoothness-gated MED-PEE -> tests/golden/pee_gate_kat.json.

Computed by the scalar restatement tests/pee_gate_scalar.py alone (not by the vectorised spec
tests/pee_gate_spec.py they then check).  Inputs are regenerated from their seeds
(codec_tcc_amd.synth + numpy default_rng), so the file holds only digests and small tables.

    python tests/golden/make_pee_gate_golden.py
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
import pee_gate_scalar as S  # noqa: E402

# (kind, h, w, seed, T, G, maxval or None, clip, payload rule)
CASES = [
    ("ct12", 32, 48, 1, 2, 24, None, False, "half"),
    ("ct12", 33, 41, 2, 1, 16, 4095, False, "half"),
    ("ct12", 40, 40, 3, 3, 32, 4095, True, "cap"),
    ("ct12", 24, 64, 4, 5, 12, 4095, True, "over"),
    ("u8", 30, 32, 5, 2, 96, None, True, "half"),
    ("u8", 31, 33, 6, 1, 0, None, True, "over"),
    ("ct12", 20, 24, 8, 2, 48, 4095, False, "zero"),
    ("ct12", 16, 24, 9, 2, 65535, 4095, True, "half"),
    ("u16", 16, 24, 10, 3, 20000, None, False, "over"),
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


def case_record(c):
    kind, h, w, seed, T, G, maxval, clip, rule = c
    img = make_image(kind, h, w, seed, maxval, clip)
    mv = int(np.iinfo(img.dtype).max) if maxval is None else maxval
    rows = img.astype(np.int64).tolist()
    _st, probe = S.embed(rows, [], T, G, mv)
    cap = probe["capacity"]
    nbits = {"zero": 0, "half": cap // 2, "cap": cap, "over": cap + 37}[rule]
    bits = payload_bits(nbits, seed).tolist()
    stego, side = S.embed(rows, bits, T, G, mv)
    got, back = S.extract(stego, side)
    assert back == rows and got == bits[:side["L"]]
    n, hs = S.table(rows, TMAX, mv)
    sel = {str(L): list(S.select(n, hs, L)) for L in (0, 1, max(1, cap // 2), cap, cap + 1, 10 ** 6)}
    return {"kind": kind, "h": h, "w": w, "seed": seed, "T": T, "G": G, "maxval": maxval, "clip": clip, "rule": rule,
            "nbits": nbits, "L": side["L"], "end": side["end"], "capacity": cap, "status": side["status"],
            "lm_count": side["lm_count"], "stego_sha256": sha(stego), "lm_sha256": sha([int(v) for v in side["lm"]]),
            "n": n, "hs": hs, "tmax": TMAX, "select": sel}


if __name__ == "__main__":
    out = {"cases": [case_record(c) for c in CASES]}
    path = os.path.join(HERE, "pee_gate_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(out["cases"]), "cases")

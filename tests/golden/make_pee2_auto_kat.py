#!/usr/bin/env python3
"""Known answers of capacity-controlled scheme 2 (T = "auto": the first T in tmin..tmax whose
four passes hold the payload, else the truncated tmax embedding) -> tests/golden/pee2_auto_kat.json.

Computed by looping the scalar restatement tests/pee_scalar.py's embed_multi over T (not by the
vectorised oracle the CPU test then checks, nor by the GPU).  Inputs are regenerated from their
seeds (codec_tcc_amd.synth + numpy default_rng), so the file holds only the chosen T, the
per-pass (L, end, status) and the stego digest.

    python tests/golden/make_pee2_auto_kat.py
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
import pee_scalar as S  # noqa: E402

# (kind, h, w, seed, tmin, tmax, maxval or None, payload rule).  Rules against full[T], the bits
# a payload longer than every pass embeds at T: "zero"; "half1" = full[1] // 2 (fits at T = 1);
# "mid" = between full[t] and full[t + 1] for t = (tmin + tmax) // 2 (a T inside the range);
# "over" = full[tmax] + 40 (nothing fits: truncated at tmax)
CASES = [
    ("ct12", 32, 48, 21, 1, 6, 4095, "half1"),
    ("ct12", 33, 41, 22, 1, 6, 4095, "mid"),
    ("ct12", 24, 31, 23, 1, 4, 4095, "over"),
    ("u8", 30, 32, 24, 2, 6, None, "half1"),
    ("u8", 27, 20, 25, 1, 5, None, "mid"),
    ("ct12", 20, 24, 26, 3, 5, 4095, "zero"),
    ("u16", 17, 24, 27, 1, 3, None, "over"),
    ("ct12", 35, 26, 28, 2, 2, 4095, "half1"),
]


def make_image(kind, h, w, seed):
    return synth.GENERATORS[kind](h, w, seed)


def payload_bits(n, seed):
    return np.random.default_rng(2000 + seed).integers(0, 2, n).astype(np.uint8)


def scan(img_rows, bits, tmin, tmax, mv):
    """The T scan over the scalar restatement: (T, stego rows, per-pass sides)."""
    for T in range(tmin, tmax + 1):
        st, sides = S.embed_multi(img_rows, bits, T, mv)
        if sum(sd["L"] for sd in sides) == len(bits):
            break
    return T, st, sides


def case_inputs(c):
    kind, h, w, seed, tmin, tmax, maxval, rule = c
    img = make_image(kind, h, w, seed)
    mv = int(np.iinfo(img.dtype).max) if maxval is None else int(maxval)
    probe = [int(b) for b in payload_bits(h * w, 77 + seed)]
    full = {T: sum(sd["L"] for sd in S.embed_multi(img.tolist(), probe, T, mv)[1]) for T in range(1, tmax + 2)}
    t = (tmin + tmax) // 2
    n = {"zero": 0, "half1": full[1] // 2, "mid": (full[t] + full[t + 1]) // 2, "over": full[tmax] + 40}[rule]
    return img, payload_bits(n, seed), mv


def main():
    out = []
    for c in CASES:
        img, bits, mv = case_inputs(c)
        blist = [int(b) for b in bits]
        T, st, sides = scan(img.tolist(), blist, c[4], c[5], mv)
        got, back = S.extract_multi(st, sides)
        L = sum(sd["L"] for sd in sides)
        assert got == blist[:L] and back == img.tolist()
        stego = np.array(st, dtype=img.dtype)
        out.append({"kind": c[0], "h": c[1], "w": c[2], "seed": c[3], "tmin": c[4], "tmax": c[5], "maxval": c[6],
                    "rule": c[7], "L_in": int(bits.size), "T": T, "L": L, "status": 1 if L < bits.size else 0,
                    "passes": [{"L": sd["L"], "end": sd["end"], "status": sd["status"]} for sd in sides],
                    "stego_sha256": hashlib.sha256(stego.tobytes()).hexdigest()})
        print(c, "-> T", T, "L", L, "of", bits.size)
    with open(os.path.join(HERE, "pee2_auto_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"{len(out)} cases -> pee2_auto_kat.json")


if __name__ == "__main__":
    main()

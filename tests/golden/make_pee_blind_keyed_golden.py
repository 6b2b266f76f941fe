#!/usr/bin/env python3
"""Known-answer vectors of keyed blind MED-PEE -> tests/golden/pee_blind_keyed_kat.json.

Computed by the scalar restatement tests/pee_blind_keyed_scalar.py alone (not by the spec
tests/pee_blind_keyed_spec.py they then check).  The covers are regenerated from their seeds
(tests/pee_blind_keyed_cases.py), so the file holds only digests, tags, header and frame words.

    python tests/golden/make_pee_blind_keyed_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pee_blind_cases as CS  # noqa: E402
import pee_blind_keyed_cases as KC  # noqa: E402
import pee_blind_keyed_scalar as KS  # noqa: E402
import pee_blind_scalar as S  # noqa: E402

CAPACITY = ("smooth", "planted1", "planted3", "wide_t4", "u8", "wide")   # small enough to try every length


def sha(rows):
    return hashlib.sha256(np.asarray(rows, dtype=np.int64).tobytes()).hexdigest()


def case_record(case):
    name, _src, T, _E, lengths, _cap = case
    img = KC.cover(name)
    mv, nbytes = CS.top(img.dtype), img.dtype.itemsize
    rows = img.astype(np.int64).tolist()
    runs = []
    for q, n in enumerate(lengths):
        bits = KC.payload(n, q).tolist()
        g = KC.index(name, q)
        stego, info, tag = KS.embed(rows, bits, T, mv, nbytes, KC.KEY, KC.NONCE, g)
        run = {"n_ct": n, "g": g, "info": list(info), "tag": tag.hex(), "stego_sha256": sha(stego)}
        if info[0] == 0:
            got, back, frame = KS.decode(stego, nbytes, KC.KEY)
            assert got == bits and back == rows and frame == (g, KC.NONCE, tag)
            run["words"] = [S._word(stego, k) for k in range(6 + info[2])]
        else:
            assert stego == rows
        runs.append(run)
    rec = {"case": name, "T": T, "maxval": mv, "cover_sha256": sha(rows), "runs": runs}
    if name in CAPACITY:
        rec["capacity"] = KS.capacity(rows, T, mv)
    return rec


def auto_record(entry):
    name, table = entry
    img = KC.cover(name)
    rows = img.astype(np.int64).tolist()
    return {"case": name, "tmax": KC.TMAX, "chosen": [[n, KS.choose(rows, n, KC.TMAX, CS.top(img.dtype))] for n, _t in table]}


def build():
    return {"key": KC.KEY.hex(), "nonce": KC.NONCE.hex(), "cases": [case_record(c) for c in KC.CASES],
            "auto": [auto_record(a) for a in KC.AUTO]}


if __name__ == "__main__":
    out = build()
    path = os.path.join(HERE, "pee_blind_keyed_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, sum(len(c["runs"]) for c in out["cases"]), "runs")

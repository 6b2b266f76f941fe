#!/usr/bin/env python3
"""Known-answer vectors of blind MED-PEE -> tests/golden/pee_blind_kat.json.

Computed by the scalar restatement tests/pee_blind_scalar.py alone (not by the vectorised spec
tests/pee_blind_spec.py they then check).  The covers are regenerated from their seeds
(tests/pee_blind_cases.py), so the file holds only digests, header words and small tables.

    python tests/golden/make_pee_blind_golden.py
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
import pee_blind_scalar as S  # noqa: E402

# (case name, n_user or None for the case's own, checksum, max_entries, with the padding pixel)
RUNS = [
    ("smooth", None, False, 256, False), ("smooth", 0, True, 256, False), ("planted1", None, True, 256, False),
    ("planted3", None, False, 256, False), ("planted3", 100, False, 2, False), ("planted3", 100, True, 3, False),
    ("wide_t2", None, True, 256, False), ("wide_t4", None, False, 256, False), ("wide_t4", None, True, 256, True),
    ("odd", None, True, 256, False), ("odd", 25, False, 256, False), ("u8", None, True, 256, False),
    ("u8", 2000, False, 256, False),
]
CAPACITY = ("odd", "wide_t2", "u8")   # the cases small enough to find the capacity by trying every length


def sha(rows):
    return hashlib.sha256(np.asarray(rows, dtype=np.int64).tobytes()).hexdigest()


def run_record(run):
    name, n_user, checksum, max_entries, pad = run
    case = next(c for c in CS.CASES if c[0] == name)
    _n, h, w, dtype, T, _k, n_case, _E, _r = case
    n = n_case if n_user is None else n_user
    img = CS.case_cover(case)
    if pad:
        img, _p = CS.with_padding(img, n, T)
    mv = CS.top(dtype)
    rows = img.astype(np.int64).tolist()
    bits = CS.payload(n, 1).tolist()
    stego, info = S.embed(rows, bits, T, mv, img.dtype.itemsize, checksum, max_entries)
    rec = {"case": name, "n_user": n, "checksum": checksum, "max_entries": max_entries, "pad": pad, "T": T,
           "maxval": mv, "info": list(info), "stego_sha256": sha(stego), "cover_sha256": sha(rows)}
    if info[0] == 0:
        got, back, hdr = S.decode(stego)
        assert got == bits and back == rows
        rec["words"] = [S._word(stego, k) for k in range(6 + info[2])]
        assert (not pad) or rec["words"][-1] == S.PAD
    else:
        assert stego == rows
    return rec


def build():
    caps = {}
    for name in CAPACITY:
        case = next(c for c in CS.CASES if c[0] == name)
        rows = CS.case_cover(case).astype(np.int64).tolist()
        caps[name] = {str(me): S.capacity(rows, case[4], CS.top(case[3]), me) for me in (256, 1)}
    return {"runs": [run_record(r) for r in RUNS], "capacity": caps}


if __name__ == "__main__":
    out = build()
    path = os.path.join(HERE, "pee_blind_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, len(out["runs"]), "runs")

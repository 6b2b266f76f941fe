#!/usr/bin/env python3
"""Known-answer vectors of gated blind MED-PEE -> tests/golden/pee_blind_gate_kat.json.

Computed by the scalar restatement tests/pee_blind_gate_scalar.py alone (not by the spec
tests/pee_blind_gate_spec.py they then check).  The covers are regenerated from their seeds
(tests/pee_blind_gate_cases.py), so the file holds only digests, header words and small tables.  The
cases are those of at most KAT_PIXELS pixels: the restatement visits one candidate at a time.

    python tests/golden/make_pee_blind_gate_golden.py
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
import pee_blind_gate_cases as GC  # noqa: E402
import pee_blind_gate_scalar as S  # noqa: E402

KAT_PIXELS = 30000


def sha(rows):
    return hashlib.sha256(np.asarray(rows, dtype=np.int64).tobytes()).hexdigest()


def kat_cases():
    return [c for c in GC.CASES if GC.cover(c[0]).size <= KAT_PIXELS]


def case_record(case):
    name, max_entries, lengths = case
    img = GC.cover(name)
    mv = CS.top(img.dtype)
    rows = img.astype(np.int64).tolist()
    rec = {"case": name, "max_entries": max_entries, "tmax": GC.TMAX, "maxval": mv, "cover_sha256": sha(rows),
           "curve": S.choose(rows, 0, GC.TMAX, mv, max_entries)[3], "runs": []}
    for q, (n, _t, _g) in enumerate(lengths):
        bits = GC.payload(n, q + 1).tolist()
        checksum = q % 2 == 0
        stego, info, T, G = S.embed(rows, bits, GC.TMAX, mv, img.dtype.itemsize, checksum, max_entries)
        run = {"n_user": n, "checksum": checksum, "T": T, "G": G, "info": list(info), "stego_sha256": sha(stego)}
        if T:
            run["words"] = [S._word(stego, k) for k in range(6 + info[2])]
        else:
            assert stego == rows
        rec["runs"].append(run)
    return rec


def build():
    return {"cases": [case_record(c) for c in kat_cases()]}


if __name__ == "__main__":
    out = build()
    path = os.path.join(HERE, "pee_blind_gate_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, sum(len(c["runs"]) for c in out["cases"]), "runs")

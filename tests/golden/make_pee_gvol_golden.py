#!/usr/bin/env python3
"""Known answers of the gated MED-PEE volume plan -> tests/golden/pee_gvol_kat.json.

Computed by the scalar restatement in tests/pee_gvol_spec.py (plan_scalar: plain loops and
ints), not by the vectorised spec the CPU test then checks, nor by the GPU.  The tables are not
written out: they are regenerated from their sources (pee_gvol_spec.source_tables -- the
synth.ct12 stacks of pee_volume_spec.BATCHES, the quadrants of tests/golden/images.npz, the
synthetic witness tables).

    python tests/golden/make_pee_gvol_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pee_gvol_spec as S  # noqa: E402

# N as a function of cap = the stack's capacity at (tmax, the open gate) -- at (tmax, g) for a
# fixed gate
RULES = {"zero": lambda cap: 0, "one": lambda cap: 1, "third": lambda cap: cap // 3, "half": lambda cap: cap // 2,
         "quarter": lambda cap: cap // 4, "cap": lambda cap: cap, "over": lambda cap: cap + 1}

# (source, tmax, g_fixed, rule or N)
CASES = [
    ("5x64x96", 16, None, "zero"), ("5x64x96", 16, None, 63), ("5x64x96", 16, None, 207), ("5x64x96", 16, None, "third"),
    ("5x64x96", 16, None, "cap"), ("5x64x96", 16, None, "over"), ("5x64x96", 16, 6, "half"), ("5x64x96", 16, 6, "over"),
    ("5x64x96", 16, 65535, "third"), ("5x64x96", 4, None, "half"),
    ("3x33x47", 16, None, "one"), ("3x33x47", 16, None, "half"), ("3x33x47", 16, None, "over"), ("3x33x47", 16, 6, "cap"),
    ("3x33x47:1", 16, None, "third"), ("3x33x47:1", 16, 0, "half"),
    ("4x32x64", 16, None, 49), ("4x32x64", 16, None, "cap"), ("4x32x64", 1, None, "half"), ("4x32x64", 16, 3, "zero"),
    ("1100x8x16", 16, None, "third"), ("1100x8x16", 16, None, "over"), ("1100x8x16", 16, 6, "half"),
    ("pe", 16, None, 4096), ("pe", 16, None, 16384), ("pe", 16, None, 32768), ("pe", 16, 6, 4096),
    ("torax", 16, None, 4096), ("torax", 16, None, 16384), ("torax", 16, None, 32768), ("torax", 16, 6, 4096),
    ("witness1", 16, None, "quarter"), ("witness1", 16, None, "half"), ("witness1", 16, None, "cap"),
    ("witness1", 16, None, "over"), ("witness2", 16, None, "third"), ("witness1", 16, 6, "half"),
]


def case_n(tables, g_fixed, rule):
    _n, hs = S.sum_tables(tables)
    cap = S.K_of(hs, len(hs), 0 if g_fixed is not None else 15)
    return int(RULES[rule](cap)) if isinstance(rule, str) else int(rule)


def main():
    out = []
    for source, tmax, g_fixed, rule in CASES:
        tables = S.source_tables(source, tmax, g_fixed)
        N = case_n(tables, g_fixed, rule)
        case = {"source": source, "tmax": tmax, "g_fixed": g_fixed, "rule": rule, "N": N, "B": len(tables)}
        for policy in S.POLICIES:
            p = S.plan_scalar(tables, N, policy, g_fixed)
            assert sum(p["n"]) == p["total"] and p["off"][-1] == p["total"]
            case[policy] = {k: p[k] for k in ("status", "T", "gate", "total", "requested", "capacity", "n", "t", "g", "off")}
        out.append(case)
        print(source, tmax, g_fixed, rule, "N", N, "->", {pol: (case[pol]["status"], case[pol]["T"], case[pol]["gate"])
                                                         for pol in S.POLICIES})
    with open(os.path.join(HERE, "pee_gvol_kat.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"{len(out)} cases -> pee_gvol_kat.json")


if __name__ == "__main__":
    main()

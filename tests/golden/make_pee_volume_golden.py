#!/usr/bin/env python3
"""Known answers of the MED-PEE volume plan, cut and reassembly -> tests/golden/pee_volume_kat.json.

Computed by the scalar restatement in tests/pee_volume_spec.py (plan_scalar, scatter_scalar,
gather_scalar: plain loops and ints), not by the vectorised spec the CPU test then checks, nor
by the GPU.  The capacity tables are written out in full (they are small), the streams are
regenerated from their seeds.

    python tests/golden/make_pee_volume_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pee_volume_spec as V  # noqa: E402


def caps_table(B, tmax, seed, top):
    """Curves non-decreasing in T, uneven across slices, with an all-zero slice when B >= 3."""
    rng = np.random.default_rng(seed)
    caps = np.cumsum(rng.integers(0, top, (B, tmax)), axis=1)
    if B >= 3:
        caps[1] = 0
    return caps.tolist()


# (B, tmax, seed, top, N rule): N as a function of S = the column sums
CASES = [
    (1, 1, 1, 40, lambda S: S[0]),
    (1, 4, 2, 40, lambda S: S[1] + 1),
    (5, 16, 3, 30, lambda S: 0),
    (5, 16, 4, 30, lambda S: 1),
    (5, 16, 5, 30, lambda S: S[6] - 1),
    (5, 16, 6, 30, lambda S: S[6]),
    (5, 16, 7, 30, lambda S: S[6] + 1),
    (7, 8, 8, 50, lambda S: S[-1]),
    (7, 8, 9, 50, lambda S: S[-1] + 9),
    (12, 3, 10, 9, lambda S: 63),
    (3, 2, 11, 2 ** 16, lambda S: S[0] // 2 + 12345),   # N * P past 2^32
]


def stream_bits(n, seed):
    return np.random.default_rng(5000 + seed).integers(0, 2, n).astype(np.uint8)


def main():
    out = []
    for B, tmax, seed, top, rule in CASES:
        caps = caps_table(B, tmax, seed, top)
        S = [sum(caps[b][k] for b in range(B)) for k in range(tmax)]
        N = int(rule(S))
        case = {"B": B, "tmax": tmax, "seed": seed, "caps": caps, "N": N}
        for policy in V.POLICIES:
            p = V.plan_scalar(caps, N, policy)
            assert sum(p["n"]) == p["total"] and all(0 <= n <= caps[b][p["T"] - 1] for b, n in enumerate(p["n"]))
            pw = max(1, (max(p["n"]) + 63) // 64)
            words = [int(w) for w in V.pack_stream(stream_bits(N, seed))]
            rows = V.scatter_scalar(words, p["n"], p["off"], pw)
            sw = max(1, (p["total"] + 63) // 64)
            back = V.gather_scalar(rows, p["n"], sw)
            want = [int(w) for w in V.pack_stream(stream_bits(N, seed)[:p["total"]])][:sw]
            assert back == want, (B, tmax, seed, policy)
            keep = {k: p[k] for k in ("status", "T", "total", "capacity", "n", "t", "off")}
            keep["payload_words"] = pw
            if B * pw <= 16:   # the rows themselves, as hex words, where they are few
                keep["rows"] = [[format(w, "016x") for w in r] for r in rows]
            case[policy] = keep
        out.append(case)
        print(B, tmax, seed, "N", N, "->", {pol: (case[pol]["T"], case[pol]["status"]) for pol in V.POLICIES})
    with open(os.path.join(HERE, "pee_volume_kat.json"), "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"{len(out)} cases -> pee_volume_kat.json")


if __name__ == "__main__":
    main()

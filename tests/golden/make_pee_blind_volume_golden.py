#!/usr/bin/env python3
"""Known-answer vectors of blind volume payloads -> tests/golden/pee_blind_volume_kat.json.

The new parts -- the curve transform, the plan, the frames, the order, the tiling and `missing` --
are computed by the scalar restatement at the end of tests/pee_blind_volume_spec.py alone (not by
plan() / frame() / order(), which they then check); the stego digests and chosen T's come from the
composition with the blind specs, whose own answers tests/golden/pee_blind_auto_kat.json pins.  The
covers are regenerated from their seeds (tests/pee_blind_volume_cases.py), so the file holds only
digests and small tables.

    python tests/golden/make_pee_blind_volume_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import pee_blind_volume_cases as VC  # noqa: E402
import pee_blind_volume_spec as VS  # noqa: E402


def sha(a):
    return hashlib.sha256(np.asarray(a, dtype=np.int64).tobytes()).hexdigest()


def words_of(bits):
    return [sum(int(bits[32 * k + j]) << j for j in range(32)) for k in range(len(bits) // 32)]


def case_record(shape, B, policy, which):
    covers = VC.stack(shape, B)
    curve = VC.curve(shape, B).tolist()
    bits = VC.bits(shape, B, which)
    N = int(bits.size)
    p = VS.plan_scalar(curve, N, policy)
    crc = VS.stream_crc(bits)
    frames = [words_of(VS.frame_bits_scalar(VC.VOLUME_ID, b, B, p["off"][b], N, crc)) if p["n"][b] else [0] * 6
              for b in range(B)]
    res = VC.result(shape, B, policy, which)
    return {"shape": shape, "B": B, "policy": policy, "length": which, "N": N, "cover_sha256": sha(covers),
            "curve_sha256": sha(curve), "status": p["status"], "T": p["T"], "capacity": p["capacity"],
            "capacity_max": p["capacity_max"], "carriers": p["carriers"], "n": p["n"], "off": p["off"], "frames": frames,
            "stream_crc": crc, "ts": [int(t) for t in res["ts"]], "stego_sha256": sha(res["stego"])}


def order_records():
    """decode-side scenarios on the frames of the u16, B = 9, even, two-thirds case"""
    res = VC.result("u16", 9, "even", "most")
    car = [b for b in range(9) if res["plan"]["n"][b] > 0]
    fr = {b: [int(v) for v in res["frames"][b]] for b in car}
    n = {b: int(res["plan"]["n"][b]) for b in car}
    other = {b: [fr[b][0] ^ 1] + fr[b][1:] for b in car}
    scen = {
        "complete_reversed": [(fr[b], n[b]) for b in car[::-1]],
        "dropped_3": [(fr[b], n[b]) for b in car if b != 3],
        "dropped_first_and_last": [(fr[b], n[b]) for b in car[1:-1]],
        "duplicate_3": [(fr[b], n[b]) for b in car] + [(fr[3], n[3])],
        "mixed": [(fr[b], n[b]) for b in car[:2]] + [(other[car[2]], n[car[2]])],
        "none": [],
        "overlap": [(fr[car[0]], n[car[0]]), (fr[car[1]][:3] + [fr[car[1]][3] - 1] + fr[car[1]][4:], n[car[1]])],
        "index_past_B": [(fr[car[0]][:1] + [9] + fr[car[0]][2:], n[car[0]])],
    }
    out = []
    for name, rows in scen.items():
        status, missing = VS.order_scalar([r[0] for r in rows], [r[1] for r in rows])
        out.append({"scenario": name, "frames": [r[0] for r in rows], "n": [r[1] for r in rows], "status": status,
                    "missing": [list(m) for m in missing]})
    return out


def build():
    return {"volume_id": VC.VOLUME_ID,
            "cases": [case_record(s, B, pol, w) for s in VC.SHAPES for B in VC.BATCHES for pol in VC.POLICIES
                      for w in VC.LENGTH_NAMES],
            "orders": order_records()}


if __name__ == "__main__":
    out = build()
    path = os.path.join(HERE, "pee_blind_volume_kat.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(path, len(out["cases"]), "cases,", len(out["orders"]), "orders")

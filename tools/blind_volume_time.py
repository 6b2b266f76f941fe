#!/usr/bin/env python3
"""Timings of blind volume payloads: whole calls between two device events, host work
and read-backs included, on 256 x 512^2 and 256 x 2048^2 ct12, the two routes taken in turns on this
same tree:

  vol_e / vol_d       embed_blind_volume(check=False) / decode_blind_volume of one stream
  slice_e / slice_d   what a caller did before: blind_capacity_curve, a read-back, the plan in numpy
                      (the same rule), the stream cut and packed per slice on the host,
                      embed_blind_auto(check=False) / decode_blind and a concatenation

Both routes are checked once to return the same bits and covers.

    python3 tools/blind_volume_time.py --json J [--rounds 5] [--reps 3] [--shapes c3,headline]
    python3 tools/blind_volume_time.py --report --json J [--out profiles/r20/blind_volume_time.txt]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--bits-per-slice", type=int, default=4096)
ap.add_argument("--tmax", type=int, default=8)
ap.add_argument("--shapes", default="c3,headline")
ap.add_argument("--json", required=True)
ap.add_argument("--report", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r20", "blind_volume_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095
ROUTES = ("vol_e", "slice_e", "vol_d", "slice_d")


def fmt(v):
    m = statistics.median(v)
    return f"median {m:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, {len(v)} rounds)"


def report():
    rows, notes, device = {}, {}, ""
    with open(args.json) as f:
        for ln in f:
            r = json.loads(ln)
            device = r.get("device", device)
            rows.setdefault((r["shape"], r["route"]), []).extend(r["ms"])
            notes[r["shape"]] = r.get("note", "")
    lines = [f"Blind volume payloads, maxval {MV}, tmax {args.tmax}; whole calls between device events, host work included, "
             f"the routes taken in turns; device: {device}"]
    for name in args.shapes.split(","):
        if not any(k[0] == name for k in rows):
            continue
        B, H, W = SHAPES[name]
        lines += ["", f"{name}: {B} x {H} x {W} ct12; {notes.get(name, '')}"]
        for route in ROUTES:
            if (name, route) in rows:
                lines.append(f"  {route:<8}: {fmt(rows[(name, route)])}")
        for a, b in (("vol_e", "slice_e"), ("vol_d", "slice_d")):
            if (name, a) in rows and (name, b) in rows:
                lines.append(f"  {a} / {b} = {statistics.median(rows[(name, a)]) / statistics.median(rows[(name, b)]):.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if args.report:
    report()
    sys.exit(0)

sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

dev = torch.device("cuda", 0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def plan_even(curve, N):
    """DESIGN §3n's rule on a host curve [B][tmax]: (n, off) per slice"""
    c = np.where(curve >= 192, curve - 192, 0).astype(np.int64)
    S = c.sum(axis=0)
    T = int(np.flatnonzero(S >= N)[0]) + 1
    P = np.concatenate([[0], np.cumsum(c[:, T - 1])]).astype(object)
    cut = [N * int(p) // int(P[-1]) for p in P]
    return [cut[b + 1] - cut[b] for b in range(len(c))], cut[:-1]


out = []
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    N = B * args.bits_per_slice
    bits = np.random.default_rng(3).integers(0, 2, N).astype(np.uint8)
    codec = PeeCodec(B, H, W, T=1, tmax=args.tmax, maxval=MV, device=dev)
    stego_v, stego_s = torch.empty_like(covers), torch.empty_like(covers)

    def vol_e():
        return codec.embed_blind_volume(covers, bits, volume_id=7, tmax=args.tmax, stego=stego_v, check=False)

    def slice_e():
        curve = codec.blind_capacity_curve(covers, tmax=args.tmax).cpu().numpy()   # the first read-back
        n, off = plan_even(curve, N)
        parts = [bits[o:o + k] for k, o in zip(n, off)]
        return codec.embed_blind_auto(covers, parts, tmax=args.tmax, stego=stego_s, check=False)

    def vol_d():
        return codec.decode_blind_volume(stego_v, verify=False)

    def slice_d():
        got, cover = codec.decode_blind(stego_s, verify=False)
        return np.concatenate(got), cover

    _s, info, ts = vol_e()
    slice_e()
    v = info["volume"].cpu().tolist()
    assert v[0] == 0, f"the stream does not fit: {v}"
    bv, cv = vol_d()
    bs, cs = slice_d()
    assert np.array_equal(bv, bits) and np.array_equal(bs, bits) and torch.equal(cv, covers) and torch.equal(cs, covers)
    th = [t for t in ts.cpu().tolist() if t]
    note = f"N = {N} bits, T* = {v[1]}, {v[4]} carriers, slice T = {min(th)}..{max(th)}; both routes return the same bits and covers"
    routes = {"vol_e": vol_e, "slice_e": slice_e, "vol_d": vol_d, "slice_d": slice_d}
    for f in routes.values():
        f()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    for k, vms in t.items():
        out.append({"shape": name, "route": k, "ms": vms, "note": note, "device": torch.cuda.get_device_name(0)})
        print(f"{name} {k}: median {statistics.median(vms):.3f} ms", flush=True)
    del covers, stego_v, stego_s, codec
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

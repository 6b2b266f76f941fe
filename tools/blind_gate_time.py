#!/usr/bin/env python3
"""Timings of gated blind MED-PEE, whole calls between two device events, on
256 x 2048^2 and 256 x 512^2 ct12, out of place, preallocated outputs, check=False:

  curve4 / curve16     blind_capacity_curve at tmax = 4 / 16: the ungated table of every T from one read
                       of the covers, and its plan (the same bytes read as the gated pass)
  gtable4 / gtable16   gate_table at tmax = 4 / 16: the roughness classes of every candidate into the
                       gated capacity table (the same classes as the gated pass)
  gcurve4 / gcurve16   blind_capacity_gated at tmax = 4 / 16: the gated table of every (T, class) per
                       candidate row and the plan over every pair
  auto_e4 / auto_e16   embed_blind_auto of the payload
  gated_e4 / gated_e16 embed_blind_gated of the same payload

One process loads one library, so the parent commit is measured by running this file on a checkout
of the parent (--tree PATH: curve*, gtable*, auto_e*) in turns with this tree's: every run appends its
rounds to --json, and --report turns the collected rounds into the table (medians and the rounds' ranges).

    python3 tools/blind_gate_time.py --label tree   --json J [--rounds 5] [--reps 5] [--shapes headline,c3]
    python3 tools/blind_gate_time.py --label parent --json J --tree /path/to/parent/checkout
    python3 tools/blind_gate_time.py --report --json J [--out profiles/r21/blind_gate_time.txt]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--bits", type=int, default=8192)
ap.add_argument("--bits-small", type=int, default=1024)
ap.add_argument("--max-entries", type=int, default=1024)
ap.add_argument("--shapes", default="headline,c3")
ap.add_argument("--label", default="tree")
ap.add_argument("--tree", default=HERE)
ap.add_argument("--json", required=True)
ap.add_argument("--report", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r21", "blind_gate_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095
TMS = (4, 16)
ROUTES = tuple(f"{r}{tm}" for r in ("curve", "gtable", "gcurve", "auto_e", "gated_e") for tm in TMS)


def fmt(v):
    m = statistics.median(v)
    return f"median {m:8.4f} ms  (min {min(v):.4f}, max {max(v):.4f}, spread {(max(v) - min(v)) / m:.3f}, {len(v)} rounds)"


def report():
    rows, notes = {}, {}
    device = ""
    with open(args.json) as f:
        for ln in f:
            r = json.loads(ln)
            device = r.get("device", device)
            rows.setdefault((r["shape"], r["label"], r["route"]), []).extend(r["ms"])
            notes[r["shape"]] = max(notes.get(r["shape"], ""), r.get("note", ""), key=len)
    lines = [f"Gated blind MED-PEE, maxval {MV}; whole calls between device events, runs of this tree and of the parent "
             f"commit taken in turns; device: {device}"]

    def med(name, label, route):
        v = rows.get((name, label, route))
        return statistics.median(v) if v else None

    for name in args.shapes.split(","):
        B, H, W = SHAPES[name]
        lines += ["", f"{name}: {B} x {H} x {W} ct12; {notes.get(name, '')}"]
        for route in ROUTES:
            for label in ("parent", "tree"):
                v = rows.get((name, label, route))
                if v:
                    lines.append(f"  {label:<6} {route:<10}: {fmt(v)}")
        for tm in TMS:
            g, c, t = med(name, "tree", f"gcurve{tm}"), med(name, "parent", f"curve{tm}"), med(name, "parent", f"gtable{tm}")
            if g and c and t:
                lines.append(f"  tmax = {tm:2}: gated table + plan = {g:.4f} ms; the parent's blind_capacity_curve {c:.4f} ms, "
                             f"gate_table {t:.4f} ms: / the larger = {g / max(c, t):.3f}, / their sum = {g / (c + t):.3f}")
            e, a = med(name, "tree", f"gated_e{tm}"), med(name, "parent", f"auto_e{tm}")
            if e and a:
                lines.append(f"  tmax = {tm:2}: embed_blind_gated / the parent's embed_blind_auto = {e / a:.3f} ({e - a:+.4f} ms)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if args.report:
    report()
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

dev = torch.device("cuda", 0)
have_gated = hasattr(PeeCodec, "embed_blind_gated")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = []
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    nbits = args.bits if name == "headline" else args.bits_small
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, nbits).astype(np.uint8) for _ in range(B)]
    codec = PeeCodec(B, H, W, T=1, maxval=MV, device=dev)
    packed = codec.pack_payloads(bits)
    stego = torch.empty_like(covers)
    note = f"{nbits} bits per slice, max_entries {args.max_entries}"
    me = args.max_entries
    if have_gated:
        st, info, ts, gs = codec.embed_blind_gated(covers, None, tmax=16, stego=stego, packed=packed, check=False, max_entries=me)
        th, gh = ts.cpu().tolist(), gs.cpu().tolist()
        assert min(th) >= 1, "a slice was refused at tmax = 16"
        got, back = codec.decode_blind(st, verify=False)
        assert torch.equal(back, covers) and all(np.array_equal(g, b) for g, b in zip(got, bits))
        gc = codec.blind_capacity_gated(covers, tmax=16, max_entries=me)
        # the last class is the ungated plan: the gated table's column 15 is the ungated curve
        assert torch.equal(gc[:, :, 15], codec.blind_capacity_curve(covers, tmax=16, max_entries=me))
        note += f"; chosen T = {min(th)}..{max(th)}, gate = {min(gh)}..{max(gh)} (tmax 16)"
    routes = {}
    for tm in TMS:
        routes[f"curve{tm}"] = lambda tm=tm: codec.blind_capacity_curve(covers, tmax=tm, max_entries=me)
        routes[f"gtable{tm}"] = lambda tm=tm: codec.gate_table(covers, tmax=tm)
        routes[f"auto_e{tm}"] = lambda tm=tm: codec.embed_blind_auto(covers, None, tmax=tm, stego=stego, packed=packed,
                                                                     check=False, max_entries=me)
        if have_gated:
            routes[f"gcurve{tm}"] = lambda tm=tm: codec.blind_capacity_gated(covers, tmax=tm, max_entries=me)
            routes[f"gated_e{tm}"] = lambda tm=tm: codec.embed_blind_gated(covers, None, tmax=tm, stego=stego, packed=packed,
                                                                           check=False, max_entries=me)
    for f in routes.values():   # warm-up: workspaces allocated, kernels loaded
        f()
        f()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            f()   # untimed: the codec keeps its last four blind workspaces, so a route may have to make its own again
            t[k].append(timed(f, args.reps))
    for k, v in t.items():
        out.append({"shape": name, "label": args.label, "route": k, "ms": v, "note": note,
                    "device": torch.cuda.get_device_name(0)})
        print(f"{name} {args.label} {k}: median {statistics.median(v):.4f} ms")
    del covers, stego, codec, routes
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

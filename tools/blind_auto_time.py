#!/usr/bin/env python3
"""Timings of blind MED-PEE with capacity control, whole calls between two device
events, on 256 x 2048^2 and 256 x 512^2 ct12, out of place, preallocated outputs, check=False:

  plan        blind_capacity at one T: the fixed row table and plan (one read of the covers)
  plan_loop8 / plan_loop16   8 / 16 such calls, T = 1 .. 8 / 16: what a caller had to do before
              (without the read-backs between them)
  curve8 / curve16   blind_capacity_curve at tmax = 8 / 16: the row table of every T from ONE read
              of the covers, and the plan that walks it
  blind_e     embed_blind at the T the auto route chooses for the payload (the largest over the
              slices, so that every slice embeds)
  auto_e8 / auto_e16   embed_blind_auto at tmax = 8 / 16 of the same payload

One process loads one library, so the parent commit is measured by running this file on a checkout
of the parent (--tree PATH: plan, plan_loop*, blind_e at the T this tree's first run chose and left
in <json>.tfixed, or --t-fixed) in turns with this tree's: every run appends its rounds to --json,
and --report turns the collected rounds into the table (medians and the rounds' ranges).

    python3 tools/blind_auto_time.py --label tree   --json J [--rounds 5] [--reps 5] [--shapes headline,c3]
    python3 tools/blind_auto_time.py --label parent --json J --tree /path/to/parent/checkout
    python3 tools/blind_auto_time.py --report --json J [--out profiles/r17/blind_auto_time.txt]
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
ap.add_argument("--t-fixed", default="", help="shape=T,... : the T of blind_e where the tree cannot choose it")
ap.add_argument("--json", required=True)
ap.add_argument("--report", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r17", "blind_auto_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095
ROUTES = ("plan", "plan_loop8", "plan_loop16", "curve8", "curve16", "blind_e", "auto_e8", "auto_e16")


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
    lines = [f"Blind MED-PEE with capacity control, maxval {MV}; whole calls between device events, runs of this tree and of "
             f"the parent commit taken in turns; device: {device}"]

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
                    lines.append(f"  {label:<6} {route:<11}: {fmt(v)}")
        for tm in (8, 16):
            c, lp, one = med(name, "tree", f"curve{tm}"), med(name, "parent", f"plan_loop{tm}"), med(name, "parent", "plan")
            if c and lp and one:
                lines.append(f"  tmax = {tm:2}: one auto pass + plan / the parent's {tm} blind_capacity calls = {c / lp:.3f}; "
                             f"/ one such call = {c / one:.2f}")
            a, e = med(name, "tree", f"auto_e{tm}"), med(name, "parent", "blind_e")
            if a and e and c and one:
                lines.append(f"  tmax = {tm:2}: embed_blind_auto - the parent's embed_blind at the chosen T = {a - e:.4f} ms; "
                             f"the table pass and plan alone differ by {c - one:.4f} ms")
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
have_auto = hasattr(PeeCodec, "embed_blind_auto")
t_fixed = {}
if os.path.exists(args.json + ".tfixed"):
    with open(args.json + ".tfixed") as f:
        t_fixed.update((k, int(v)) for k, v in (ln.split("=") for ln in f.read().split()))
t_fixed.update((k, int(v)) for k, v in (kv.split("=") for kv in args.t_fixed.split(",") if kv))


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
    fixed = {T: PeeCodec(B, H, W, T=T, maxval=MV, device=dev) for T in range(1, 17)}
    codec = fixed[1]
    packed = codec.pack_payloads(bits)
    stego = torch.empty_like(covers)
    note = f"{nbits} bits per slice, max_entries {args.max_entries}"
    if have_auto:
        st, info, ts = codec.embed_blind_auto(covers, None, tmax=16, stego=stego, packed=packed, check=False,
                                              max_entries=args.max_entries)
        th = ts.cpu().tolist()
        assert min(th) >= 1, "a slice was refused at tmax = 16"
        got, back = codec.decode_blind(st, verify=False)
        assert torch.equal(back, covers) and all(np.array_equal(g, b) for g, b in zip(got, bits))
        curve = codec.blind_capacity_curve(covers, tmax=16, max_entries=args.max_entries).cpu().numpy()
        for T in (1, 2, 8, 16):   # the table's columns are the fixed plan's capacities
            assert curve[:, T - 1].tolist() == fixed[T].blind_capacity(covers, args.max_entries).cpu().tolist(), T
        tf = max(th)
        st8, _i8, ts8 = codec.embed_blind_auto(covers, None, tmax=8, packed=packed, check=False, max_entries=args.max_entries)
        note += f"; chosen T = {min(th)}..{tf} (tmax 16), {min(ts8.cpu().tolist())}..{max(ts8.cpu().tolist())} (tmax 8)"
        with open(args.json + ".tfixed", "a") as f:   # the parent's runs read it (--t-fixed overrides)
            f.write(f"{name}={tf}\n")
    else:
        tf = t_fixed[name]
    routes = {"plan": lambda: fixed[2].blind_capacity(covers, args.max_entries),
              "plan_loop8": lambda: [fixed[T].blind_capacity(covers, args.max_entries) for T in range(1, 9)],
              "plan_loop16": lambda: [fixed[T].blind_capacity(covers, args.max_entries) for T in range(1, 17)],
              "blind_e": lambda: fixed[tf].embed_blind(covers, None, stego=stego, packed=packed, check=False,
                                                       max_entries=args.max_entries)}
    if have_auto:
        routes.update({
            "curve8": lambda: codec.blind_capacity_curve(covers, tmax=8, max_entries=args.max_entries),
            "curve16": lambda: codec.blind_capacity_curve(covers, tmax=16, max_entries=args.max_entries),
            "auto_e8": lambda: codec.embed_blind_auto(covers, None, tmax=8, stego=stego, packed=packed, check=False,
                                                      max_entries=args.max_entries),
            "auto_e16": lambda: codec.embed_blind_auto(covers, None, tmax=16, stego=stego, packed=packed, check=False,
                                                       max_entries=args.max_entries)})
    for f in routes.values():   # warm-up: workspaces allocated, kernels loaded
        f()
        f()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    for k, v in t.items():
        out.append({"shape": name, "label": args.label, "route": k, "ms": v, "note": note,
                    "device": torch.cuda.get_device_name(0)})
        print(f"{name} {args.label} {k}: median {statistics.median(v):.4f} ms")
    del covers, stego, codec, fixed, routes
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

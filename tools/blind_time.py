#!/usr/bin/env python3
"""Blind MED-PEE timings, whole calls between two device events, on 256 x 2048^2 and
256 x 512^2 ct12 at T = 2, out of place, preallocated outputs, check=False:

  roi     embed + extract with the last two pixel rows protected (codec_pee_roi_embed /
          codec_pee_roi_extract): the step the blind one is built around
  blind   embed_blind + decode_blind (checksum=False, verify=False): the row table, the plan, the
          splice, the same ROI embed, the pack; the header gather with its read-back, the scatter,
          the same ROI extract, the restore, the payload read-back
  plan    blind_capacity alone: the row table and the plan (one read-only pass over the covers)
  roi_e / blind_e   the embed halves of the two steps alone (no read-back in either)

The payload is --bits per slice where the covers hold it, else --bits-small (the 512^2 slices hold
about 2000 bits at T = 2).  One process loads one library, so the parent commit's roi step is
measured by running this file on a checkout of the parent (--tree PATH; only `roi` is measured
when that tree has no blind entries) in turns with this tree's: every run appends its rounds to
--json, and --report turns the collected rounds into the table (medians and the rounds' ranges).

    python3 tools/blind_time.py --label tree   --json J [--rounds 5] [--reps 5] [--shapes headline,c3]
    python3 tools/blind_time.py --label parent --json J --tree /path/to/parent/checkout
    python3 tools/blind_time.py --report --json J [--out profiles/r16/blind_time.txt]
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
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r16", "blind_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095


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
    lines = [f"Blind MED-PEE timings, T = 2, maxval {MV}; whole calls between device events, runs of this tree and of the "
             f"parent commit taken in turns; device: {device}"]
    for name in args.shapes.split(","):
        B, H, W = SHAPES[name]
        lines += ["", f"{name}: {B} x {H} x {W} ct12; {notes.get(name, '')}"]
        for label, route in (("parent", "roi"), ("tree", "roi"), ("tree", "blind"), ("parent", "roi_e"), ("tree", "roi_e"),
                             ("tree", "blind_e"), ("tree", "plan")):
            v = rows.get((name, label, route))
            if v:
                lines.append(f"  {label:<6} {route:<6}: {fmt(v)}")
        pr, tr, tb = (rows.get((name, a, b)) for a, b in (("parent", "roi"), ("tree", "roi"), ("tree", "blind")))
        if pr and tr:
            lines.append(f"  roi step, tree / parent = {statistics.median(tr) / statistics.median(pr):.3f} (the same objects)")
        if pr and tb:
            lines.append(f"  blind step / parent roi step = {statistics.median(tb) / statistics.median(pr):.3f} (informational)")
        pe, be, pl = (rows.get((name, a, b)) for a, b in (("parent", "roi_e"), ("tree", "blind_e"), ("tree", "plan")))
        if pe and be and pl:
            lines.append(f"  blind embed - parent roi embed = {statistics.median(be) - statistics.median(pe):.4f} ms; the row table "
                         f"and the plan alone take {statistics.median(pl):.4f} ms (informational)")
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
from codec_tcc_amd import _lib  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

dev = torch.device("cuda", 0)
have_blind = hasattr(PeeCodec, "embed_blind")


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
    codec = PeeCodec(B, H, W, T=2, maxval=MV, device=dev)
    nbits = args.bits
    if have_blind and int(codec.blind_capacity(covers, args.max_entries).min().item()) < nbits:
        nbits = args.bits_small
    elif not have_blind and name == "c3":
        nbits = args.bits_small
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, nbits).astype(np.uint8) for _ in range(B)]
    packed = codec.pack_payloads(bits)
    pw = packed[0].shape[1]
    stego, back = torch.empty_like(covers), torch.empty_like(covers)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device=dev)
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=dev)
    outw = torch.empty((B, pw), dtype=torch.int64, device=dev)
    rect = codec.pack_roi((H - 2, 0, H, W))

    def roi():
        codec.embed(covers, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False, roi=rect)
        codec.extract(stego, meta, lm, payload_words=pw, cover=back, payload=outw, roi=True)

    routes = {"roi": roi, "roi_e": lambda: codec.embed(covers, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False,
                                                       roi=rect)}
    note = f"{nbits} bits per slice"
    if have_blind:
        def blind():
            st, _info = codec.embed_blind(covers, None, stego=stego, packed=packed, check=False, max_entries=args.max_entries)
            codec.decode_blind(st, cover=back, verify=False)

        routes.update({"blind": blind, "plan": lambda: codec.blind_capacity(covers, args.max_entries),
                       "blind_e": lambda: codec.embed_blind(covers, None, stego=stego, packed=packed, check=False,
                                                            max_entries=args.max_entries)})
        st, info = codec.embed_blind(covers, None, stego=stego, packed=packed, check=False, max_entries=args.max_entries)
        ih = info.cpu().numpy()
        assert (ih[:, 0] == 0).all(), "a slice was refused"
        got, _c = codec.decode_blind(st, cover=back, verify=False)
        assert torch.equal(back, covers) and all(np.array_equal(g, b) for g, b in zip(got, bits))
        note += f"; E = {int(ih[:, 2].min())}..{int(ih[:, 2].max())} entries, region from row {int(ih[:, 5].min())}"
    for k, f in routes.items():   # warm-up, and exactness of what is timed
        f()
        f()
        if k in ("roi", "blind"):
            assert torch.equal(back, covers), k
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    for k, v in t.items():
        out.append({"shape": name, "label": args.label, "route": k, "ms": v, "note": note,
                    "device": torch.cuda.get_device_name(0)})
        print(f"{name} {args.label} {k}: median {statistics.median(v):.4f} ms")
    del covers, stego, back, codec
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

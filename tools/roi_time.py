#!/usr/bin/env python3
"""ROI-protected MED-PEE timings, whole calls between two device events, on
256 x 2048^2 and 256 x 512^2 ct12, 1 KB of payload per slice, out of place, preallocated
outputs, check=False:

  gated   embed + extract at T = 2, G = 24 (codec_pee_gate_embed / codec_pee_gate_extract)
  roi     the same step with a central rectangle covering a quarter of every slice
          (codec_pee_roi_embed / codec_pee_roi_extract)
  bbox    roi_bbox(covers, level) (codec_roi_bbox) ...
  crc     ... against crc32_slices(covers) on the same bytes: both are read-only streams

One process loads one library, so the parent commit's gated step is measured by running this
file on a checkout of the parent (--tree PATH: the package is imported from there; only `gated`
is measured when that tree has no ROI) in turns with this tree's: every run appends its rounds
to --json, and --report turns the collected rounds into the table (medians, the rounds' ranges,
and the verdicts: this tree's gated step within the parent's median plus the parent's
round-to-round spread; bbox against crc within that run's spread).

    python3 tools/roi_time.py --label tree   --json J [--rounds 5] [--reps 5] [--shapes headline,c3]
    python3 tools/roi_time.py --label parent --json J --tree /path/to/parent/checkout
    python3 tools/roi_time.py --report --json J [--out profiles/r13/roi_time.txt]
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
ap.add_argument("--gate", type=int, default=24)
ap.add_argument("--shapes", default="headline,c3")
ap.add_argument("--label", default="tree")
ap.add_argument("--tree", default=HERE)
ap.add_argument("--json", required=True)
ap.add_argument("--report", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r13", "roi_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV, NBITS = 4095, 8192


def fmt(v):
    m = statistics.median(v)
    return f"median {m:8.4f} ms  (min {min(v):.4f}, max {max(v):.4f}, spread {(max(v) - min(v)) / m:.3f}, {len(v)} rounds)"


def report():
    rows = {}
    device = ""
    with open(args.json) as f:
        for ln in f:
            r = json.loads(ln)
            device = r.get("device", device)
            rows.setdefault((r["shape"], r["label"], r["route"]), []).extend(r["ms"])
    lines = [f"ROI-protected MED-PEE timings, {NBITS} bits per slice, T = 2, G = {args.gate}, maxval {MV}; whole calls between "
             f"device events, runs of this tree and of the parent commit taken in turns; device: {device}"]
    for name in args.shapes.split(","):
        B, H, W = SHAPES[name]
        lines += ["", f"{name}: {B} x {H} x {W} ct12"]
        for label, route in (("parent", "gated"), ("tree", "gated"), ("tree", "roi"), ("tree", "crc"), ("tree", "bbox")):
            v = rows.get((name, label, route))
            if v:
                lines.append(f"  {label:<6} {route:<6}: {fmt(v)}")
        pg, tg, tr = (rows.get((name, a, b)) for a, b in (("parent", "gated"), ("tree", "gated"), ("tree", "roi")))
        if pg and tg:
            bound = statistics.median(pg) + (max(pg) - min(pg))
            ok = statistics.median(tg) <= bound
            lines.append(f"  1. gated step, tree / parent = {statistics.median(tg) / statistics.median(pg):.3f}; bound (parent median + "
                         f"its rounds' range) {bound:.4f} ms: {'within' if ok else 'EXCEEDED'}")
        if pg and tr:
            lines.append(f"  2. ROI step / parent gated step = {statistics.median(tr) / statistics.median(pg):.3f} (informational)")
        bb, cr = rows.get((name, "tree", "bbox")), rows.get((name, "tree", "crc"))
        if bb and cr:
            bound = statistics.median(cr) + max(max(cr) - min(cr), max(bb) - min(bb))
            ok = statistics.median(bb) <= bound
            lines.append(f"  3. roi_bbox / crc32_slices = {statistics.median(bb) / statistics.median(cr):.3f}; bound (crc median + the run's "
                         f"spread) {bound:.4f} ms: {'within' if ok else 'EXCEEDED'}")
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
from codec_tcc_amd import _lib, checksum  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

dev = torch.device("cuda", 0)
have_roi = hasattr(PeeCodec, "pack_roi")


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
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, NBITS).astype(np.uint8) for _ in range(B)]
    codec = PeeCodec(B, H, W, T=2, maxval=MV, gate=args.gate, device=dev)
    packed = codec.pack_payloads(bits)
    pw = packed[0].shape[1]
    stego, back = torch.empty_like(covers), torch.empty_like(covers)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device=dev)
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=dev)
    outw = torch.empty((B, pw), dtype=torch.int64, device=dev)

    def gated():
        codec.embed(covers, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False)
        codec.extract(stego, meta, lm, payload_words=pw, cover=back, payload=outw)

    routes = {"gated": gated}
    if have_roi:
        from codec_tcc_amd.roi import roi_bbox
        rect = codec.pack_roi((H // 4, W // 4, 3 * H // 4, 3 * W // 4))   # a quarter of the slice, central

        def roi():
            codec.embed(covers, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False, roi=rect)
            codec.extract(stego, meta, lm, payload_words=pw, cover=back, payload=outw, roi=True)

        crc_out = checksum.crc32_slices(covers)
        level = int(covers[0].to(torch.int32).max().item()) // 2   # (no uint16 reductions in torch)
        routes.update({"roi": roi, "crc": lambda: checksum.crc32_slices(covers, out=crc_out),
                       "bbox": lambda: roi_bbox(covers, level=level)})
    for k, f in routes.items():   # exactness of what is timed, and warm-up
        f()
        f()
        if k in ("gated", "roi"):
            assert torch.equal(back, covers), k
    if have_roi:
        y0, x0, y1, x1 = H // 4, W // 4, 3 * H // 4, 3 * W // 4
        routes["roi"]()
        for b in (0, B // 2, B - 1):   # (compared on the host: torch has few uint16 kernels for strided views)
            assert np.array_equal(stego[b, y0:y1, x0:x1].cpu().numpy(), covers[b, y0:y1, x0:x1].cpu().numpy()), b
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    for k, v in t.items():
        out.append({"shape": name, "label": args.label, "route": k, "ms": v, "device": torch.cuda.get_device_name(0)})
        print(f"{name} {args.label} {k}: median {statistics.median(v):.4f} ms")
    del covers, stego, back, codec
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

#!/usr/bin/env python3
"""Keyed MED-PEE timings, whole calls between two device events, on 256 x 2048^2
and 256 x 512^2 ct12, 1 KB of payload per slice at 2048^2 and 256 bytes at 512^2 (what every slice holds at
T = 2: a truncated slice does not authenticate), out of place, preallocated outputs, check=False:

  step      unkeyed embed + extract at T = 2 (what every tree has)
  keyed     encrypt + tag + embed, then extract + tag + release (this tree)
  crc       crc32_slices(covers) ...
  poly      ... against poly1305_tags(ctx, covers) on the same bytes (an empty CT)
  copy      a device copy of one 256 MB row ...
  chacha0/1 ... against chacha20_rows on that row, layout 0 (a lane owns a block) and 1 (a quad
            owns a block); measured once, on the first shape

One process loads one library, so the parent commit's step is measured by running this file on
a checkout of the parent (--tree PATH; only `step` is measured there) in turns with this tree's:
every run appends its rounds to --json, and --report turns the collected rounds into the table.

    python3 tools/aead_time.py --label tree   --json J [--rounds 5] [--reps 5] [--shapes headline,c3]
    python3 tools/aead_time.py --label parent --json J --tree /path/to/parent/checkout
    python3 tools/aead_time.py --report --json J [--out profiles/r14/aead_time.txt]
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
ap.add_argument("--shapes", default="headline,c3")
ap.add_argument("--label", default="tree")
ap.add_argument("--tree", default=HERE)
ap.add_argument("--json", required=True)
ap.add_argument("--report", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r14", "aead_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095
NBITS = {"headline": 8192, "c3": 2048}
ROW_BYTES = 256 << 20
PEAK_TBS = 8.0   # the chip's HBM rate the fractions are quoted against


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
    lines = [f"Keyed MED-PEE timings, {NBITS['headline']} / {NBITS['c3']} bits per slice at 2048^2 / 512^2, T = 2, maxval {MV}; whole calls between device events, runs of "
             f"this tree and of the parent commit taken in turns; measured on an AMD Instinct MI355X (gfx950), whose "
             f"name the runtime reports as '{device}'.  Informational: no pass mark."]
    for name in args.shapes.split(","):
        B, H, W = SHAPES[name]
        nbytes = B * H * W * 2
        lines += ["", f"{name}: {B} x {H} x {W} ct12 ({nbytes / 2 ** 20:.0f} MiB of covers)"]
        for label, route in (("parent", "step"), ("tree", "step"), ("tree", "keyed"), ("tree", "crc"), ("tree", "poly"),
                             ("tree", "copy"), ("tree", "chacha0"), ("tree", "chacha1")):
            v = rows.get((name, label, route))
            if v:
                extra = ""
                m = statistics.median(v) * 1e-3
                if route in ("crc", "poly"):
                    extra = f"  {nbytes / m / 1e12:.2f} TB/s read = {nbytes / m / 1e12 / PEAK_TBS:.2f} of {PEAK_TBS:.0f} TB/s"
                if route in ("copy", "chacha0", "chacha1"):
                    extra = (f"  {2 * ROW_BYTES / m / 1e12:.2f} TB/s read + written = "
                             f"{2 * ROW_BYTES / m / 1e12 / PEAK_TBS:.2f} of {PEAK_TBS:.0f} TB/s")
                lines.append(f"  {label:<6} {route:<8}: {fmt(v)}{extra}")
        ps, ts, tk = (rows.get((name, a, b)) for a, b in (("parent", "step"), ("tree", "step"), ("tree", "keyed")))
        if ps and ts:
            lines.append(f"  unkeyed step, tree / parent = {statistics.median(ts) / statistics.median(ps):.3f} (parent's rounds' "
                         f"range {max(ps) - min(ps):.4f} ms)")
        if ts and tk:
            lines.append(f"  keyed step / unkeyed step = {statistics.median(tk) / statistics.median(ts):.3f}")
        cr, po = rows.get((name, "tree", "crc")), rows.get((name, "tree", "poly"))
        if cr and po:
            lines.append(f"  poly1305_tags / crc32_slices = {statistics.median(po) / statistics.median(cr):.3f}")
        cp = rows.get((name, "tree", "copy"))
        for k in ("chacha0", "chacha1"):
            v = rows.get((name, "tree", k))
            if cp and v:
                lines.append(f"  {k} / copy = {statistics.median(v) / statistics.median(cp):.3f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if args.report:
    report()
    sys.exit(0)

os.environ.setdefault("CODEC_TUNING", "1")   # the layout knob below is honoured only under the tuning switch
sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from codec_tcc_amd import _lib, checksum  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

dev = torch.device("cuda", 0)
try:
    from codec_tcc_amd import aead
except ImportError:
    aead = None
KEY, NONCE = bytes(range(32)), bytes(range(8))


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
first = True
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, NBITS[name]).astype(np.uint8) for _ in range(B)]
    codec = PeeCodec(B, H, W, T=2, maxval=MV, device=dev)
    words, lengths, lens_t = codec.pack_payloads(bits)
    pw = words.shape[1]
    stego, back = torch.empty_like(covers), torch.empty_like(covers)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device=dev)
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=dev)
    outw = torch.empty((B, pw), dtype=torch.int64, device=dev)

    def step():
        codec.embed(covers, None, stego=stego, lm=lm, meta=meta, packed=(words, lengths, lens_t), check=False)
        codec.extract(stego, meta, lm, payload_words=pw, cover=back, payload=outw)

    routes = {"step": step}
    if aead is not None:
        ctx = aead.upload_ctx(KEY, NONCE, dev)
        ct, pt = torch.empty_like(words), torch.empty_like(words)
        tag, tag2 = (torch.empty((B, 4), dtype=torch.int32, device=dev) for _ in range(2))
        ok = torch.empty(B, dtype=torch.int32, device=dev)
        crc_out = checksum.crc32_slices(covers)

        def keyed():
            aead.chacha20_rows(ctx, words, lens_t, 0, out=ct)
            aead.poly1305_tags(ctx, covers, ct, lens_t, 0, out=tag)
            codec.embed(covers, None, stego=stego, lm=lm, meta=meta, packed=(ct, lengths, lens_t), check=False)
            codec.extract(stego, meta, lm, payload_words=pw, cover=back, payload=outw)
            aead.poly1305_tags(ctx, back, outw, lens_t, 0, out=tag2)
            aead.release(ctx, tag2, tag, outw, lens_t, 0, out=pt, ok=ok)

        routes.update({"keyed": keyed, "crc": lambda: checksum.crc32_slices(covers, out=crc_out),
                       "poly": lambda: aead.poly1305_tags(ctx, covers, out=tag)})
        if first:
            row = torch.empty((1, ROW_BYTES // 8), dtype=torch.int64, device=dev).random_()
            row_out = torch.empty_like(row)
            row_len = torch.tensor([2 ** 31 - 1], dtype=torch.int32, device=dev)

            def chacha(v):
                def run():
                    os.environ["CODEC_CHACHA_VARIANT"] = str(v)
                    aead.chacha20_rows(ctx, row, row_len, aead.STREAM_INDEX, out=row_out)
                return run

            routes.update({"copy": lambda: row_out.copy_(row), "chacha0": chacha(0), "chacha1": chacha(1)})
    for k, f in routes.items():   # exactness of what is timed, and warm-up
        f()
        f()
        if k in ("step", "keyed"):
            assert torch.equal(back, covers), k
        if k == "keyed":
            assert bool(ok.all().item()) and torch.equal(pt, words), k
    if aead is not None and first:   # the two layouts write the same bytes
        routes["chacha0"]()
        a = row_out.clone()
        routes["chacha1"]()
        assert torch.equal(a, row_out) and not torch.equal(a, row)
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    os.environ.pop("CODEC_CHACHA_VARIANT", None)
    for k, v in t.items():
        out.append({"shape": name, "label": args.label, "route": k, "ms": v, "device": torch.cuda.get_device_name(0)})
        print(f"{name} {args.label} {k}: median {statistics.median(v):.4f} ms")
    first = False
    del covers, stego, back, codec
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

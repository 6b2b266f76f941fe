#!/usr/bin/env python3
"""Keyed blind MED-PEE timings, whole calls between two device events, on 256 x 2048^2
and 256 x 512^2 ct12 at T = 2, out of place, preallocated stego, check=False:

  blind_e   embed_blind (checksum=False): the unkeyed step
  blind_d   decode_blind (verify=False): header gather and read-back, extract, payload read-back
  chacha    chacha20_rows over the payload rows alone
  poly      poly1305_tags over (covers, ciphertext rows) alone
  release   aead.release over the ciphertext rows alone
  keyed_e   embed_blind_keyed: context upload, chacha20_rows, poly1305_tags, frames, the keyed embed
  keyed_d   decode_blind_keyed: header gather and read-back, extract, unframe, poly1305_tags_n over
            the restored covers, release_n, one read-back
  keyed_d0  decode_blind_keyed(verify=False): chacha20_rows_n in place of the tag pass and release

--report sets keyed_e beside blind_e + chacha + poly and keyed_d beside blind_d + poly + release.

    python3 tools/blind_keyed_time.py --json J [--rounds 5] [--reps 5] [--shapes headline,c3]
    python3 tools/blind_keyed_time.py --report --json J [--out profiles/r18/blind_keyed_time.txt]
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
ap.add_argument("--json", required=True)
ap.add_argument("--report", action="store_true")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r18", "blind_keyed_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV, T = 4095, 2
ROUTES = ("blind_e", "blind_d", "chacha", "poly", "release", "keyed_e", "keyed_d", "keyed_d0")


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
            rows.setdefault((r["shape"], r["route"]), []).extend(r["ms"])
            notes[r["shape"]] = r.get("note", "")
    lines = [f"Keyed blind MED-PEE, T = {T}, maxval {MV}; whole calls between device events; device: {device}"]
    for name in args.shapes.split(","):
        B, H, W = SHAPES[name]
        lines += ["", f"{name}: {B} x {H} x {W} ct12; {notes.get(name, '')}"]
        med = {}
        for route in ROUTES:
            v = rows.get((name, route))
            if v:
                med[route] = statistics.median(v)
                lines.append(f"  {route:<9}: {fmt(v)}")
        if all(k in med for k in ("keyed_e", "blind_e", "chacha", "poly")):
            parts = med["blind_e"] + med["chacha"] + med["poly"]
            lines.append(f"  keyed_e - (blind_e + chacha + poly) = {med['keyed_e'] - parts:+.4f} ms ({med['keyed_e'] / parts:.3f} of the sum)")
        if all(k in med for k in ("keyed_d", "blind_d", "poly", "release")):
            parts = med["blind_d"] + med["poly"] + med["release"]
            lines.append(f"  keyed_d - (blind_d + poly + release) = {med['keyed_d'] - parts:+.4f} ms ({med['keyed_d'] / parts:.3f} of the sum)")
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
from codec_tcc_amd import aead  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

dev = torch.device("cuda", 0)
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
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    nbits = args.bits if name == "headline" else args.bits_small
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, nbits).astype(np.uint8) for _ in range(B)]
    codec = PeeCodec(B, H, W, T=T, maxval=MV, device=dev)
    packed = codec.pack_payloads(bits)
    words, _lengths, lens_t = packed
    stego, kstego, back = torch.empty_like(covers), torch.empty_like(covers), torch.empty_like(covers)
    kw = dict(packed=packed, check=False, max_entries=args.max_entries)
    codec.embed_blind(covers, None, stego=stego, **kw)
    _st, info, _ts = codec.embed_blind_keyed(covers, None, key=KEY, nonce=NONCE, stego=kstego, **kw)
    assert not info[:, 0].any().item(), "a slice was refused"
    got, rest = codec.decode_blind_keyed(kstego, KEY, cover=back)
    assert torch.equal(rest, covers) and all(np.array_equal(g, b) for g, b in zip(got, bits))
    ctx = aead.upload_ctx(KEY, NONCE, dev)
    ct = aead.chacha20_rows(ctx, words, lens_t)
    tags = aead.poly1305_tags(ctx, covers, ct, lens_t)
    pt = torch.empty_like(ct)
    note = f"{nbits} bits per slice, max_entries {args.max_entries}"
    routes = {"blind_e": lambda: codec.embed_blind(covers, None, stego=stego, **kw),
              "blind_d": lambda: codec.decode_blind(stego, cover=back, verify=False),
              "chacha": lambda: aead.chacha20_rows(ctx, words, lens_t, out=ct),
              "poly": lambda: aead.poly1305_tags(ctx, covers, ct, lens_t, out=tags),
              "release": lambda: aead.release(ctx, tags, tags, ct, lens_t, out=pt),
              "keyed_e": lambda: codec.embed_blind_keyed(covers, None, key=KEY, nonce=NONCE, stego=kstego, **kw),
              "keyed_d": lambda: codec.decode_blind_keyed(kstego, KEY, cover=back),
              "keyed_d0": lambda: codec.decode_blind_keyed(kstego, KEY, cover=back, verify=False)}
    for f in routes.values():   # warm-up: workspaces allocated, kernels loaded
        f()
        f()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    for k, v in t.items():
        out.append({"shape": name, "route": k, "ms": v, "note": note, "device": torch.cuda.get_device_name(0)})
        print(f"{name} {k}: median {statistics.median(v):.4f} ms")
    del covers, stego, kstego, back, codec, routes
    torch.cuda.empty_cache()

with open(args.json, "a") as f:
    for r in out:
        f.write(json.dumps(r) + "\n")

"""Tile-checksum pass times on the MI355X (HIP events, medians), against the slice pass on the
same bytes in the same process:

    python tools/tile_crc_time.py [--out profiles/r12/tile_crc_time.txt] [--reps 20] [--small]
                                  [--steps-only]

Legs, alternated launch by launch inside one timed loop:
  codec_crc32_slices (the yardstick: same bytes, same lookups per byte)
  codec_crc32_tiles at each tile size of the case
Cases: 256 x 2048^2 uint16 at tiles 64, 32, 128; 256 x 512^2 uint16 at tile 64 (rotated over 8
copies so that no launch re-reads what the Infinity Cache still holds); 256 x 2048^2 uint8 at
tile 64 and uint16 at tile 32 are the 64-B-segment access shapes.
Then, host clock around synchronised steps as DESIGN §3d's figures were taken: embed with
checksum=False / True / "tiles", and decode (verify=True) of an unaltered checksum=True
encoding -- the leg that runs unchanged on a tree without tile checksums, so the same tool run on
both trees gives the pair (--steps-only skips the kernel legs, and "tiles" where it is unknown).
Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="B = 8 (a rehearsal, not a measurement)")
    ap.add_argument("--steps-only", action="store_true", help="only the embed / decode step times")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/tile_crc_time.py needs a GPU")
    import bench
    from codec_tcc_amd import checksum, pee
    have_tiles = hasattr(checksum, "crc32_tiles")
    dev = torch.device("cuda", 0)
    B = 8 if args.small else 256
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/tile_crc_time.py: B = {B}, {args.reps} timed launches per leg (alternated), medians; device "
        f"{torch.cuda.get_device_name(0)}; tile checksums {'present' if have_tiles else 'absent (parent tree)'}")

    def kernel_case(H, dtype, tiles, copies):
        W = H
        if dtype == "uint16":
            bufs = [bench.make_covers(torch, "ct12", B, H, W, dev, s) for s in range(copies)]
        else:
            g = torch.Generator(device=dev).manual_seed(7)
            bufs = [torch.randint(0, 256, (B, H, W), generator=g, device=dev, dtype=torch.uint8) for _ in range(copies)]
        nbytes = bufs[0].numel() * bufs[0].element_size()
        crc_out = torch.empty(B, dtype=torch.int32, device=dev)
        outs = {t: torch.empty((B,) + checksum.tile_grid(H, W, t), dtype=torch.int32, device=dev) for t in tiles}
        legs = {"codec_crc32_slices": lambda x: checksum.crc32_slices(x, out=crc_out)}
        for t in tiles:
            legs[f"codec_crc32_tiles tile {t} (route {checksum.tiles_route(bufs[0], t)})"] = \
                (lambda tt: lambda x: checksum.crc32_tiles(x, tt, out=outs[tt]))(t)
        for fn in legs.values():
            for x in bufs:
                fn(x)
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for r in range(args.reps):
            for k, fn in legs.items():
                x = bufs[r % copies]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(x)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        say()
        say(f"## {B} x {H}^2 {dtype} = {nbytes / 1e6:.0f} MB" + (f" (rotated over {copies} copies)" if copies > 1 else ""))
        base = float(np.median(times["codec_crc32_slices"]))
        for k, t in times.items():
            m = float(np.median(t))
            say(f"{k:48s} {m:8.4f} ms  {nbytes / m / 1e6:8.1f} GB/s  {nbytes / m * 1e3 / PEAK:6.3f} of 8 TB/s  "
                f"x{m / base:5.2f} of the slice pass  (min {min(t):.4f}, max {max(t):.4f})")
        del bufs, outs
        torch.cuda.empty_cache()

    if have_tiles and not args.steps_only:
        kernel_case(2048, "uint16", (64, 32, 128), 1)
        kernel_case(512, "uint16", (64,), 8)
        kernel_case(2048, "uint8", (64,), 1)

    # ---- the embed and decode steps (host clock, synchronised)
    for H, copies in ((2048, 1), (512, 8)):
        W = H
        bufs = [bench.make_covers(torch, "ct12", B, H, W, dev, s) for s in range(copies)]
        codec = pee.PeeCodec(B, H, W, dtype="uint16", T=2, maxval=4095)
        rng = np.random.default_rng(1)
        payloads = [rng.integers(0, 2, 4096, dtype=np.uint8) for _ in range(B)]
        stego = torch.empty_like(bufs[0])
        enc_true = codec.embed(bufs[0], payloads, checksum=True)
        steps = {"embed, checksum=False": lambda x: codec.embed(x, payloads, stego=stego),
                 "embed, checksum=True": lambda x: codec.embed(x, payloads, stego=stego, checksum=True)}
        if have_tiles:
            steps['embed, checksum="tiles" (tile 64)'] = lambda x: codec.embed(x, payloads, stego=stego, checksum="tiles")
        steps["decode of an unaltered checksum=True encoding, verify=True"] = lambda x: codec.decode(enc_true, verify=True)
        for fn in steps.values():
            fn(bufs[0])
        torch.cuda.synchronize()
        st = {k: [] for k in steps}
        for r in range(max(5, args.reps // 2)):
            for k, fn in steps.items():
                x = bufs[r % copies]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(x)
                torch.cuda.synchronize()
                st[k].append((time.perf_counter() - t0) * 1e3)
        say()
        say(f"## steps, {B} x {H}^2 uint16 (host clock, synchronised)")
        base = float(np.median(st["embed, checksum=True"]))
        for k, t in st.items():
            m = float(np.median(t))
            rel = f"  {m - base:+8.3f} ms on checksum=True" if k.startswith("embed") else ""
            say(f"{k:60s} {m:8.3f} ms{rel}  (min {min(t):.3f}, max {max(t):.3f})")
        del bufs, stego, codec, enc_true
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""CRC-32 pass and checksummed MED-PEE step times on the MI355X (HIP events, medians):

    python tools/crc_bench.py [--out profiles/r08/crc_time.txt] [--reps 20] [--small]

Two batches of uint16 ct12 slices, 256 x 2048^2 (2.1 GB) and 256 x 512^2 (134 MB; rotated over
8 copies so that no launch re-reads what the Infinity Cache still holds).  Legs, alternated
launch by launch inside one timed loop:
  codec_crc32_slices with each table layout (CODEC_CRC_VARIANT 0..3, the library's A/B knob)
  codec_pee_capacity on the same batch -- the existing read-only pass over the same bytes
  the PEE embed + decode step with checksum=True / verify=True and without (host clock around
  the step; decode ends in the payload read-back, i.e. a device synchronise)
Reports GB/s, the fraction of the 8 TB/s HBM peak and both ratios.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["CODEC_TUNING"] = "1"   # the layout knob is read only under the tuning switch

VARIANTS = {0: "plain table, 256 threads", 1: "8 copies, 256 threads", 2: "32 copies (one per bank), 1024 threads",
            3: "plain table, 1024 threads"}
PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="B = 8 (a rehearsal, not a measurement)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/crc_bench.py needs a GPU")
    import bench
    from codec_tcc_amd import _lib, checksum, pee
    lib = _lib.load()
    lib.codec_set_tuning(1)
    default_variant = 1
    dev = torch.device("cuda", 0)
    B = 8 if args.small else 256
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say(f"# tools/crc_bench.py: B = {B}, {args.reps} timed launches per leg (alternated), medians; device "
        f"{torch.cuda.get_device_name(0)}")
    for H, copies in ((2048, 1), (512, 8)):
        W = H
        nbytes = B * H * W * 2
        bufs = [bench.make_covers(torch, "ct12", B, H, W, dev, s) for s in range(copies)]
        codec = pee.PeeCodec(B, H, W, dtype="uint16", T=2, maxval=4095)
        outs = torch.empty(B, dtype=torch.int32, device=dev)

        def crc_leg(v):
            def run(x):
                os.environ["CODEC_CRC_VARIANT"] = str(v)
                checksum.crc32_slices(x, out=outs)
            return run
        legs = {f"crc32 variant {v} ({VARIANTS[v]})": crc_leg(v) for v in VARIANTS}
        legs["codec_pee_capacity"] = lambda x: codec.capacity(x)
        for fn in legs.values():   # warm-up: every leg on every buffer
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
        os.environ["CODEC_CRC_VARIANT"] = str(default_variant)
        say()
        say(f"## {B} x {H}^2 uint16 = {nbytes / 1e6:.0f} MB" + (f" (rotated over {copies} copies)" if copies > 1 else ""))
        cap = float(np.median(times["codec_pee_capacity"]))
        for k, t in times.items():
            m = float(np.median(t))
            say(f"{k:58s} {m:8.4f} ms  {nbytes / m / 1e6:8.1f} GB/s  {nbytes / m * 1e3 / PEAK:6.3f} of 8 TB/s  "
                f"x{m / cap:5.2f} of the capacity pass  (min {min(t):.4f}, max {max(t):.4f})")

        # ---- the embed + decode step, with and without checksums
        rng = np.random.default_rng(1)
        payloads = [rng.integers(0, 2, 4096, dtype=np.uint8) for _ in range(B)]
        stego = torch.empty_like(bufs[0])

        def step(ck):
            def run(x):
                enc = codec.embed(x, payloads, stego=stego, checksum=ck)
                codec.decode(enc, verify=ck)
            return run
        steps = {"PEE embed + decode, no checksums": step(False), "PEE embed + decode, checksum=True / verify=True": step(True)}
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
        base = float(np.median(st["PEE embed + decode, no checksums"]))
        for k, t in st.items():
            m = float(np.median(t))
            say(f"{k:58s} {m:8.3f} ms (host clock, synchronised)  x{m / base:5.3f} of the step without  "
                f"(min {min(t):.3f}, max {max(t):.3f})")
        del bufs, stego, codec
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

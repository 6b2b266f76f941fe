#!/usr/bin/env python3
"""Smoothness-gated MED-PEE against the ungated calls, interleaved round by round in one process,
on C3 (256 x 512^2 ct12) and the headline shape (256 x 2048^2), 1 KB of payload per slice, out
of place, preallocated outputs, check=False:

  (a) embed + extract at T = 2: ungated (codec_pee_embed_ts / codec_pee_extract) against the
      gate G = 24 (codec_pee_gate_embed / codec_pee_gate_extract);
  (b) embed with capacity control: embed(T="auto") (codec_pee_embed_auto) against
      gate="auto", T="auto" (codec_pee_gate_embed_auto: table + selection + embed);
  (c) the table pass alone: capacity() (codec_pee_capacity) against gate_table()
      (codec_pee_gate_capacity), which read the same bytes.

Every step is timed as whole calls (host work included) between two device events, the second
followed by a synchronise; medians of alternating rounds with the rounds' ranges.  Writes --out
(default profiles/r10/gate_time.txt).  The ungated side is this build's; whether it is the
parent commit's is bench.py's question (profiles/r10/bench_pairs.txt).

    python3 tools/gate_time.py [--rounds 9] [--reps 5] [--shapes c3,headline] [--out PATH]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from codec_tcc_amd import _lib  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--gate", type=int, default=24)
ap.add_argument("--shapes", default="c3,headline")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "r10", "gate_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV, NBITS = 4095, 8192
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


def fmt(v):
    return f"median {statistics.median(v):8.4f} ms  (min {min(v):.4f}, max {max(v):.4f}, spread {(max(v) - min(v)) / statistics.median(v):.3f})"


lines = [f"gated vs ungated MED-PEE, {NBITS} bits per slice, G = {args.gate}, maxval {MV}; {args.rounds} alternating "
         f"rounds x {args.reps} calls; device: {torch.cuda.get_device_name(0)}"]
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    rng = np.random.default_rng(3)
    bits = [rng.integers(0, 2, NBITS).astype(np.uint8) for _ in range(B)]
    codecs = {"plain": PeeCodec(B, H, W, T=2, maxval=MV, device=dev),
              "gated": PeeCodec(B, H, W, T=2, maxval=MV, gate=args.gate, device=dev),
              "auto": PeeCodec(B, H, W, T="auto", maxval=MV, device=dev),
              "gauto": PeeCodec(B, H, W, T="auto", maxval=MV, gate="auto", device=dev)}
    packed = codecs["plain"].pack_payloads(bits)
    pw = packed[0].shape[1]
    stego, back = torch.empty_like(covers), torch.empty_like(covers)
    lm = torch.empty((B, codecs["plain"].lm_words), dtype=torch.int64, device=dev)
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=dev)
    outw = torch.empty((B, pw), dtype=torch.int64, device=dev)

    def embed(k):
        return lambda: codecs[k].embed(covers, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False)

    def step(k):
        def f():
            codecs[k].embed(covers, None, stego=stego, lm=lm, meta=meta, packed=packed, check=False)
            codecs[k].extract(stego, meta, lm, payload_words=pw, cover=back, payload=outw)
        return f

    routes = {"a ungated embed+extract T=2": step("plain"), f"a gated   embed+extract T=2 G={args.gate}": step("gated"),
              "b embed(T=auto)": embed("auto"), "b embed(T=auto, gate=auto)": embed("gauto"),
              "c capacity()": lambda: codecs["auto"].capacity(covers), "c gate_table()": lambda: codecs["gauto"].gate_table(covers)}
    # exactness of what is timed: both steps restore the covers, and the payload rows wherever the
    # slice held its payload (a 512^2 slice at T = 2 does not hold 1 KB: truncated, status 1)
    full = {}
    for k in ("plain", "gated"):
        step(k)()
        raw = meta.cpu().numpy().tobytes()
        ok = np.array([_lib.PeeMeta.from_buffer_copy(raw, i * _lib.PEE_META_BYTES).status == 0 for i in range(B)])
        full[k] = int(ok.sum())
        same = (outw.cpu().numpy() == packed[0].cpu().numpy().view(np.int64))[ok].all()
        assert torch.equal(back, covers) and same, k
    embed("gauto")()
    ts, gs = codecs["gauto"].t_slices.cpu().numpy(), codecs["gauto"].g_slices.cpu().numpy()
    embed("auto")()
    t0 = codecs["auto"].t_slices.cpu().numpy()
    for f in routes.values():
        for _ in range(2):
            f()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            t[k].append(timed(f, args.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    keys = list(routes)
    lines += ["", f"{name}: {B} x {H} x {W} ct12, row pitch {pw} words; slices holding the whole payload at T = 2: "
              f"ungated {full['plain']}, gated {full['gated']} of {B}; T='auto' picks "
              f"{ {int(v): int((t0 == v).sum()) for v in np.unique(t0)} }, gate='auto' picks (T, G) "
              f"{ {(int(a), int(b)): int(((ts == a) & (gs == b)).sum()) for a, b in sorted(set(zip(ts.tolist(), gs.tolist())))} }"]
    lines += [f"  ({k[0]}) {k[2:]:<36}: {fmt(t[k])}" for k in keys]
    lines += [f"  (a) gated / ungated = {med[keys[1]] / med[keys[0]]:.3f}   (b) gated / ungated = {med[keys[3]] / med[keys[2]]:.3f}   "
              f"(c) table / capacity = {med[keys[5]] / med[keys[4]]:.3f}"]
    del covers, stego, back, codecs
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))

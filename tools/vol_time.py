#!/usr/bin/env python3
"""One payload across a slice stack, three ways, interleaved round by round in one process, on
C3 (256 x 512^2 ct12) and the headline shape (256 x 2048^2), N = 2 097 152 bits:

  (a) PeeCodec.embed_volume + decode_volume: plan, cut and reassembly on the device;
  (b) the same job on the per-slice interface: capacity(), read-back, the plan in numpy,
      pack_payloads, embed(T="auto") with those lengths (it picks the same per-slice T);
      decode() and host concatenation.  Its stego, records and bits must equal (a)'s;
  (c) embed(T="auto") + decode() with N / B bits per slice: the floor without any planning.

Every route is timed as a whole call (host work included) between two device events, the
second followed by a synchronise; medians of alternating rounds with the rounds' ranges, and
the embed and decode halves separately.  Writes --out (default profiles/r09/vol_time.txt).

    python3 tools/vol_time.py [--rounds 9] [--reps 5] [--bits 2097152] [--policy even] [--out PATH]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from codec_tcc_amd.pee import PeeCodec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--bits", type=int, default=2097152)
ap.add_argument("--policy", default="even")
ap.add_argument("--tmax", type=int, default=16)
ap.add_argument("--shapes", default="c3,headline")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "r09", "vol_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095
dev = torch.device("cuda", 0)
N = args.bits
bits = np.random.default_rng(9).integers(0, 2, N).astype(np.uint8)


def host_plan(caps, N, policy):
    """The rule of include/codec_tcc_vol.h in numpy (int64: N * P < 2^62): n per slice."""
    S = caps.sum(axis=0)
    hit = np.flatnonzero(S >= N)
    T = int(hit[0]) + 1 if hit.size else caps.shape[1]
    N = N if hit.size else int(S[-1])
    c = caps[:, T - 1].astype(np.int64)
    P = np.concatenate([[0], np.cumsum(c)])
    if policy == "even":
        cut = N * P // P[-1] if P[-1] else np.zeros_like(P)
        return np.diff(cut)
    return np.minimum(c, np.maximum(0, N - P[:-1]))


def timed(fn, reps):
    """Mean ms per call of fn() over reps calls, by device events around the whole loop."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fmt(v):
    return f"median {statistics.median(v):8.4f} ms  (min {min(v):.4f}, max {max(v):.4f})"


lines = [f"volume payload of {N} bits, policy {args.policy}, tmax {args.tmax}, maxval {MV}; "
         f"{args.rounds} alternating rounds x {args.reps} calls; device: {torch.cuda.get_device_name(0)}"]
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    vc = PeeCodec(B, H, W, dtype="uint16", tmax=args.tmax, maxval=MV, device=dev)
    ac = PeeCodec(B, H, W, dtype="uint16", T="auto", tmax=args.tmax, maxval=MV, device=dev)
    stego = torch.empty_like(covers)
    keep = {}

    def a_embed():
        keep["vol"] = vc.embed_volume(covers, bits, policy=args.policy, stego=stego)

    def a_decode():
        keep["a_out"] = vc.decode_volume(keep["vol"])

    def b_embed():
        caps = ac.capacity(covers).cpu().numpy()
        n = host_plan(caps, N, args.policy)
        off = np.concatenate([[0], np.cumsum(n)])
        keep["enc"] = ac.embed(covers, [bits[off[b]:off[b + 1]] for b in range(B)], stego=stego)

    def b_decode():
        per, cover = ac.decode(keep["enc"])
        keep["b_out"] = (np.concatenate(per), cover)

    share = [bits[b * (N // B):(b + 1) * (N // B)] for b in range(B)]

    def c_embed():
        keep["cenc"] = ac.embed(covers, share, stego=stego)

    def c_decode():
        keep["c_out"] = ac.decode(keep["cenc"])

    # (a) and (b) must agree bit for bit
    a_embed()
    a_stego, a_recs = stego.clone(), [(r.T, r.L, r.end, r.status) for r in keep["vol"].enc.records()]
    plan = keep["vol"].plan_host()
    a_decode()
    b_embed()
    same = bool(torch.equal(a_stego.view(torch.uint8), stego.view(torch.uint8))) and \
        a_recs == [(r.T, r.L, r.end, r.status) for r in keep["enc"].records()]
    b_decode()
    same = same and np.array_equal(keep["a_out"][0], keep["b_out"][0]) and np.array_equal(keep["a_out"][0], bits) and \
        bool(torch.equal(keep["a_out"][1].view(torch.uint8), keep["b_out"][1].view(torch.uint8)))
    del a_stego
    c_embed()
    c_decode()
    routes = {"a": (a_embed, a_decode), "b": (b_embed, b_decode), "c": (c_embed, c_decode)}
    for e, d in routes.values():   # warm every shape the timed windows use
        for _ in range(2):
            e()
            d()
    t = {k: {"embed": [], "decode": []} for k in routes}
    for _ in range(args.rounds):
        for k, (e, d) in routes.items():
            t[k]["embed"].append(timed(e, args.reps))
            t[k]["decode"].append(timed(d, args.reps))
    tot = {k: [x + y for x, y in zip(t[k]["embed"], t[k]["decode"])] for k in routes}
    med = {k: statistics.median(tot[k]) for k in routes}
    spread = {k: (max(tot[k]) - min(tot[k])) / med[k] for k in routes}
    ts = plan["t"]
    lines += [
        "",
        f"{name}: {B} x {H} x {W} ct12; T* = {plan['T']}, status {plan['status']}, per-slice T "
        f"{ {int(v): int((ts == v).sum()) for v in np.unique(ts)} }, n_b {int(plan['n'].min())} .. {int(plan['n'].max())}, "
        f"row pitch {keep['vol'].enc.payload_words} words (b: {keep['enc'].payload_words})",
        f"  (a) = (b) bit for bit (stego, records, bits, covers): {same}",
    ]
    for k, label in (("a", "embed_volume + decode_volume"), ("b", "capacity + numpy plan + embed/decode"),
                     ("c", "embed/decode, N/B bits per slice")):
        lines += [f"  ({k}) {label:<38}: {fmt(tot[k])}",
                  f"        embed {fmt(t[k]['embed'])}",
                  f"        decode {fmt(t[k]['decode'])}"]
    lines += [f"  (a)/(b) = {med['a'] / med['b']:.3f}   (a)/(c) = {med['a'] / med['c']:.3f}   "
              f"spread of the rounds (max - min) / median: a {spread['a']:.3f}, b {spread['b']:.3f}, c {spread['c']:.3f}",
              f"  embed only: (a)/(b) = {statistics.median(t['a']['embed']) / statistics.median(t['b']['embed']):.3f}, "
              f"decode only: (a)/(b) = {statistics.median(t['a']['decode']) / statistics.median(t['b']['decode']):.3f}"]
    del covers, stego, keep, vc, ac
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))

#!/usr/bin/env python3
"""One payload across a slice stack with the smoothness gate, three ways, interleaved round by
round in one process (the method of tools/vol_time.py), on C3 (256 x 512^2 ct12) and the
headline shape (256 x 2048^2), N = 2 097 152 bits:

  (a) PeeCodec.embed_volume(gate="auto") + decode_volume: table, plan over (T, G), cut, gated
      embed, gated extract and reassembly on the device;
  (b) the ungated embed_volume + decode_volume: what the gate costs on top of the volume call;
  (c) the gated job of (a) on the per-slice interface: gate_table(), read-back, the rule of
      include/codec_tcc_gvol.h on the host, pack_payloads, codec_pee_gate_embed with the planned
      T_b and G_b; decode() and host concatenation.  Its stego, records and bits must equal (a)'s.

Every route is timed as a whole call (host work included) between two device events, the
second followed by a synchronise; medians of alternating rounds with the rounds' ranges, and
the embed and decode halves separately.  Writes --out (default profiles/r11/gvol_time.txt).

    python3 tools/gvol_time.py [--rounds 7] [--reps 3] [--bits 2097152] [--policy even] [--out PATH]
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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--bits", type=int, default=2097152)
ap.add_argument("--policy", default="even")
ap.add_argument("--tmax", type=int, default=16)
ap.add_argument("--shapes", default="c3,headline")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                              "profiles", "r11", "gvol_time.txt"))
args = ap.parse_args()

SHAPES = {"c3": (256, 512, 512), "headline": (256, 2048, 2048)}
MV = 4095
GATES = np.array(_lib.GATES, dtype=np.int64)
dev = torch.device("cuda", 0)
N = args.bits
bits = np.random.default_rng(9).integers(0, 2, N).astype(np.uint8)


def _curves(n, hs):
    """K[.., T - 1, j], A[.., T - 1, j] of tables n[.., 16], hs[.., tmax, 16] (int64 / object)."""
    tmax = hs.shape[-2]
    u = np.arange(tmax)
    cost = (u * u + (u + 1) * (u + 1)).reshape(tmax, 1)
    K = np.cumsum(np.cumsum(hs, axis=-2), axis=-1)
    S = np.cumsum(np.cumsum(hs * cost, axis=-2), axis=-1)
    Nn = np.cumsum(n, axis=-1)[..., None, :]
    T2 = (2 * (u + 1) * (u + 1)).reshape(tmax, 1)
    return K, T2 * (Nn - K) + S


def host_plan(n, hs, N, policy):
    """The rule of include/codec_tcc_gvol.h on the host: the volume choice in Python ints (its
    products pass 64 bits), the shares, and the per-slice choices as one vectorised walk over
    the 256 pairs (products below 2^62).  Returns n_b, T_b, G_b."""
    B, tmax = hs.shape[0], hs.shape[1]
    K, A = _curves(n.sum(axis=0).astype(object), hs.sum(axis=0).astype(object))
    best = None
    for T in range(1, tmax + 1):
        for j in range(16):
            k, a = int(K[T - 1][j]), int(A[T - 1][j])
            if N == 0:
                best = best or (a, k, T, j)
            elif k >= N and (best is None or a * best[1] < best[0] * k):
                best = (a, k, T, j)
    if best is None:
        best, N = (0, 0, tmax, 15), int(K[tmax - 1][15])
    Kb, Ab = _curves(n.astype(np.int64), hs.astype(np.int64))
    c = Kb[:, best[2] - 1, best[3]]
    P = np.concatenate([[0], np.cumsum(c)])
    if policy == "even":
        share = np.diff(N * P // P[-1]) if P[-1] else np.zeros(B, np.int64)
    else:
        share = np.minimum(c, np.maximum(0, N - P[:-1]))
    have = np.zeros(B, bool)
    bA, bK = np.zeros(B, np.int64), np.ones(B, np.int64)
    bT, bJ = np.ones(B, np.int64), np.zeros(B, np.int64)
    for T in range(1, tmax + 1):
        for j in range(16):
            k, a = Kb[:, T - 1, j], Ab[:, T - 1, j]
            take = np.where(share == 0, ~have, (k >= share) & (~have | (a * bK < bA * k)))
            have |= take
            bA, bK = np.where(take, a, bA), np.where(take, k, bK)
            bT, bJ = np.where(take, T, bT), np.where(take, j, bJ)
    return share, bT, GATES[bJ]


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


def rec_key(r):
    return (r.T, r.L, r.end, r.status, r.reserved[1])


lines = [f"gated volume payload of {N} bits, policy {args.policy}, tmax {args.tmax}, maxval {MV}; "
         f"{args.rounds} alternating rounds x {args.reps} calls; device: {torch.cuda.get_device_name(0)}"]
for name in args.shapes.split(","):
    B, H, W = SHAPES[name]
    covers = bench.make_covers(torch, "ct12", B, H, W, dev, seed=1000)
    vc = PeeCodec(B, H, W, dtype="uint16", tmax=args.tmax, maxval=MV, device=dev)
    gc = PeeCodec(B, H, W, dtype="uint16", T=1, tmax=args.tmax, maxval=MV, device=dev, gate=0)
    stego = torch.empty_like(covers)
    keep = {}

    def a_embed():
        keep["vol"] = vc.embed_volume(covers, bits, policy=args.policy, stego=stego, gate="auto")

    def a_decode():
        keep["a_out"] = vc.decode_volume(keep["vol"])

    def b_embed():
        keep["uvol"] = vc.embed_volume(covers, bits, policy=args.policy, stego=stego)

    def b_decode():
        keep["b_out"] = vc.decode_volume(keep["uvol"])

    def c_embed():
        n_t, hs_t = gc.gate_table(covers, args.tmax)
        host = torch.cat([n_t.reshape(-1), hs_t.reshape(-1)]).cpu().numpy().astype(np.int64)
        share, tb, gb = host_plan(host[:B * 16].reshape(B, 16), host[B * 16:].reshape(B, args.tmax, 16), N, args.policy)
        off = np.concatenate([[0], np.cumsum(share)])
        tg = torch.from_numpy(np.stack([tb, gb]).astype(np.int32)).to(dev)
        gc.t_slices.copy_(tg[0])
        gc.g_slices.copy_(tg[1])
        keep["enc"] = gc.embed(covers, [bits[off[b]:off[b + 1]] for b in range(B)], stego=stego)

    def c_decode():
        per, cover = gc.decode(keep["enc"])
        keep["c_out"] = (np.concatenate(per), cover)

    # (a) and (c) must agree bit for bit
    a_embed()
    a_stego, a_recs = stego.clone(), [rec_key(r) for r in keep["vol"].enc.records()]
    plan = keep["vol"].plan_host()
    a_decode()
    c_embed()
    same = bool(torch.equal(a_stego.view(torch.uint8), stego.view(torch.uint8))) and \
        a_recs == [rec_key(r) for r in keep["enc"].records()]
    c_decode()
    same = same and np.array_equal(keep["a_out"][0], keep["c_out"][0]) and np.array_equal(keep["a_out"][0], bits) and \
        bool(torch.equal(keep["a_out"][1].view(torch.uint8), keep["c_out"][1].view(torch.uint8)))
    del a_stego
    b_embed()
    uplan = keep["uvol"].plan_host()
    b_decode()
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
    ts, gs = plan["t"], plan["g"]
    lines += [
        "",
        f"{name}: {B} x {H} x {W} ct12; (T*, G*) = ({plan['T']}, {plan['gate']}), status {plan['status']}, capacity there "
        f"{plan['capacity']}; per-slice T { {int(v): int((ts == v).sum()) for v in np.unique(ts)} }, per-slice G "
        f"{ {int(v): int((gs == v).sum()) for v in np.unique(gs)} }, n_b {int(plan['n'].min())} .. {int(plan['n'].max())}, "
        f"row pitch {keep['vol'].enc.payload_words} words; the ungated plan: T* = {uplan['T']}",
        f"  (a) = (c) bit for bit (stego, records with their gates, bits, covers): {same}",
    ]
    for k, label in (("a", "embed_volume(gate='auto') + decode_volume"), ("b", "ungated embed_volume + decode_volume"),
                     ("c", "gate_table + host plan + gated embed/decode")):
        lines += [f"  ({k}) {label:<44}: {fmt(tot[k])}",
                  f"        embed {fmt(t[k]['embed'])}",
                  f"        decode {fmt(t[k]['decode'])}"]
    lines += [f"  (a)/(b) = {med['a'] / med['b']:.3f}   (a)/(c) = {med['a'] / med['c']:.3f}   "
              f"spread of the rounds (max - min) / median: a {spread['a']:.3f}, b {spread['b']:.3f}, c {spread['c']:.3f}",
              f"  embed only: (a)/(b) = {statistics.median(t['a']['embed']) / statistics.median(t['b']['embed']):.3f}, "
              f"(a)/(c) = {statistics.median(t['a']['embed']) / statistics.median(t['c']['embed']):.3f}; "
              f"decode only: (a)/(b) = {statistics.median(t['a']['decode']) / statistics.median(t['b']['decode']):.3f}, "
              f"(a)/(c) = {statistics.median(t['a']['decode']) / statistics.median(t['c']['decode']):.3f}"]
    del covers, stego, keep, vc, gc
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))

"""Specification of MED-PEE volume payloads (scheme 1): how one bitstream of N bits is planned
across a stack of B slices, cut into per-slice payload rows and put together again.  TEST
INFRASTRUCTURE ONLY: the HIP kernels (codec_tcc_amd/csrc/codec_vol.hip) are checked bit-exact
against plan() / scatter() / gather(), and those against the scalar restatement below (plain
Python loops and ints, as tests/pee_scalar.py is for the pixel scheme).

Inputs: caps[B][tmax] from oracle.pee_cpu.capacity_curve per slice, N, a policy.  All integer.
  S(T)   = sum_b caps[b][T-1];  T* = the smallest T in 1..tmax with S(T) >= N.  No T fits:
           status 1, T* = tmax and N is replaced by S(tmax) (the stream's first S(tmax) bits are
           embedded, as the per-slice truncation does).
  c_b    = caps[b][T*-1];  P_b = the exclusive prefix sum of c;  P_B = S(T*).
  "even" n_b = floor(N P_(b+1) / P_B) - floor(N P_b / P_B), all zero when P_B = 0.  The sum
         telescopes to N, and n_b <= c_b whenever N <= P_B: N c_b / P_B <= c_b and the two floors
         differ by less than N c_b / P_B + 1, an integer below c_b + 1.
  "fill" n_b = min(c_b, max(0, N - P_b)).
  T_b    = the smallest T with caps[b][T-1] >= n_b (codec_pee_capacity's rule: n_b = 0 gives 1);
           never above T*, where the capacity is c_b >= n_b.
  off_b  = the exclusive prefix sum of n: slice b carries stream bits [off_b, off_b + n_b).
Streams and rows are LSB-first in 64-bit words (framing.pack_bits' packing); row bits at or above
n_b are zero, and so are the gathered stream's pad bits.
Bounds: B (H//2) (W//2) <= 2^31 - 1 and 0 <= N <= 2^31 - 1, so N P < 2^62.
Row pitch: payload_words = max(1, min(ceil(N / 64), lm_words)).
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

POLICIES = ("even", "fill")
NMAX = 2 ** 31 - 1


def payload_words(N: int, lm_words: int) -> int:
    return max(1, min((int(N) + 63) // 64, int(lm_words)))


def plan(caps, N: int, policy: str = "even") -> Dict:
    """caps: [B][tmax] integers.  Returns status, T (= T*), total (the bits planned), requested,
    capacity (= S(T*)), n[B], t[B], off[B + 1] (numpy int64)."""
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {POLICIES}")
    caps = np.asarray(caps, dtype=np.int64)
    if caps.ndim != 2 or caps.shape[0] < 1 or caps.shape[1] < 1 or (caps < 0).any():
        raise ValueError("caps must be [B][tmax] with B, tmax >= 1 and no negative entry")
    N = int(N)
    if not 0 <= N <= NMAX:
        raise ValueError("N must be in 0..2^31 - 1")
    B, tmax = caps.shape
    S = caps.sum(axis=0)
    hit = np.flatnonzero(S >= N)
    status = 0 if hit.size else 1
    T = int(hit[0]) + 1 if hit.size else tmax
    requested = N
    if status:
        N = int(S[tmax - 1])
    c = caps[:, T - 1]
    P = np.concatenate([[0], np.cumsum(c)]).astype(object)   # Python ints: N * P exactly
    PB = int(P[B])
    if policy == "even":
        cut = [N * int(p) // PB if PB else 0 for p in P]
        n = np.array([cut[b + 1] - cut[b] for b in range(B)], dtype=np.int64)
    else:
        n = np.array([min(int(c[b]), max(0, N - int(P[b]))) for b in range(B)], dtype=np.int64)
    t = np.array([int(np.flatnonzero(caps[b] >= n[b])[0]) + 1 for b in range(B)], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return {"status": status, "T": T, "total": N, "requested": requested, "capacity": PB, "policy": policy,
            "n": n, "t": t, "off": off}


def pack_stream(bits, words: int | None = None) -> np.ndarray:
    """0/1 vector -> uint64 words, LSB first (framing.pack_bits' packing), zero padded."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    need = max(1, (bits.size + 63) // 64)
    words = max(need, words or 0)
    buf = np.zeros(words * 64, np.uint8)
    buf[:bits.size] = bits
    return np.packbits(buf, bitorder="little").view(np.uint64)


def unpack_stream(words, nbits: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:int(nbits)]


def scatter(stream_words, n: Sequence[int], off: Sequence[int], pw: int) -> np.ndarray:
    """rows [B][pw] uint64: row b = stream bits [off_b, off_b + n_b), zero above."""
    allbits = np.unpackbits(np.ascontiguousarray(stream_words).view(np.uint8), bitorder="little")
    rows = np.zeros((len(n), pw), np.uint64)
    for b, (nb, ob) in enumerate(zip(n, off)):
        nb, ob = int(nb), int(ob)
        if nb > 64 * pw:
            raise ValueError(f"slice {b}: {nb} bits do not fit a row of {pw} words")
        rows[b] = pack_stream(allbits[ob:ob + nb], pw)
    return rows


def gather(rows, lengths: Sequence[int], words: int) -> np.ndarray:
    """The inverse: the first lengths[b] bits of every row concatenated, packed into `words`
    uint64 words with zero pad bits (bits past 64 * words are cut)."""
    rows = np.ascontiguousarray(rows)
    parts = [unpack_stream(rows[b], int(nb)) for b, nb in enumerate(lengths)]
    bits = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if words < 1:
        return np.zeros(0, np.uint64)
    return pack_stream(bits[:64 * words], words)[:words]


def record_offsets(L: Sequence[int], pw: int, nc: int) -> np.ndarray:
    """Decode-side offsets from the records' L as the library bounds them: a negative L counts
    as 0, and L is capped at min(64 * pw, nc)."""
    lim = min(64 * int(pw), int(nc))
    x = [min(max(int(v), 0), lim) for v in L]
    return np.concatenate([[0], np.cumsum(x)]).astype(np.int64)


# ---------------------------------------------------------------- the tests' batches
# name -> (B, H, W, first seed, the saturated (all-4095) slice or None): synth.ct12 slices
BATCHES = {"5x64x96": (5, 64, 96, 100, 1), "3x33x47": (3, 33, 47, 100, 1), "4x32x64": (4, 32, 64, 100, 1),
           "1100x8x16": (1100, 8, 16, 200, None)}


def ct12_batch(name: str) -> np.ndarray:
    from codec_tcc_amd import synth
    B, H, W, seed, sat = BATCHES[name]
    covers = np.stack([synth.ct12(H, W, seed + i) for i in range(B)])
    if sat is not None:
        covers[sat] = 4095
    return covers


def curves(covers: np.ndarray, tmax: int, maxval=None) -> np.ndarray:
    from oracle import pee_cpu
    return np.stack([pee_cpu.capacity_curve(c, tmax, maxval) for c in covers])


def stream_bits(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(5000 + seed).integers(0, 2, int(n)).astype(np.uint8)


def oracle_embed(covers: np.ndarray, bits: np.ndarray, p: Dict, maxval=None):
    """The oracle driven by a plan: per slice pee_cpu.pee_embed of its share at its T.
    Returns (stegos, sides)."""
    from oracle import pee_cpu
    out = []
    for b, c in enumerate(covers):
        lo, nb = int(p["off"][b]), int(p["n"][b])
        out.append(pee_cpu.pee_embed(c, bits[lo:lo + nb], int(p["t"][b]), maxval))
    return np.stack([st for st, _ in out]), [sd for _, sd in out]


# ---------------------------------------------------------------- scalar restatement
def plan_scalar(caps: List[List[int]], N: int, policy: str = "even") -> Dict:
    """plan() in plain Python loops and ints."""
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {POLICIES}")
    B, tmax = len(caps), len(caps[0])
    S = [0] * tmax
    for b in range(B):
        for k in range(tmax):
            S[k] += int(caps[b][k])
    requested = N = int(N)
    T, status = 0, 0
    for k in range(tmax):
        if S[k] >= N:
            T = k + 1
            break
    if T == 0:
        T, status, N = tmax, 1, S[tmax - 1]
    PB = S[T - 1]
    n, t, off = [], [], [0]
    Pb = 0
    for b in range(B):
        c = int(caps[b][T - 1])
        if policy == "even":
            nb = (N * (Pb + c) // PB - N * Pb // PB) if PB else 0
        else:
            nb = min(c, max(0, N - Pb))
        Pb += c
        tb = 1
        while int(caps[b][tb - 1]) < nb:
            tb += 1
        n.append(nb)
        t.append(tb)
        off.append(off[-1] + nb)
    return {"status": status, "T": T, "total": N, "requested": requested, "capacity": PB, "policy": policy,
            "n": n, "t": t, "off": off}


def scatter_scalar(stream_words: Sequence[int], n: Sequence[int], off: Sequence[int], pw: int) -> List[List[int]]:
    """scatter() bit by bit on Python ints."""
    rows = []
    for nb, ob in zip(n, off):
        row = [0] * pw
        for k in range(int(nb)):
            p = int(ob) + k
            bit = (int(stream_words[p >> 6]) >> (p & 63)) & 1
            row[k >> 6] |= bit << (k & 63)
        rows.append(row)
    return rows


def gather_scalar(rows: Sequence[Sequence[int]], lengths: Sequence[int], words: int) -> List[int]:
    """gather() bit by bit on Python ints."""
    out = [0] * words
    p = 0
    for row, nb in zip(rows, lengths):
        for k in range(int(nb)):
            if p < 64 * words:
                out[p >> 6] |= ((int(row[k >> 6]) >> (k & 63)) & 1) << (p & 63)
            p += 1
    return out

"""Specification of gated MED-PEE volume payloads (scheme 1): how one bitstream of N bits is
planned across a stack of B slices over (T, G).  TEST INFRASTRUCTURE ONLY: the HIP kernel
(codec_tcc_amd/csrc/codec_gvol.hip, k_gvol_plan) is checked bit-exact against plan(), and that
against the scalar restatement below (plan_scalar: plain Python loops, ints and lists, as
pee_volume_spec.plan_scalar is for the ungated plan).

Inputs: per slice the gated capacity table (n_b[16], hs_b[tmax][16]) of tests/pee_gate_spec.py
(table()), with K_b(T, j), N_b(j) and A_b(T, j) as defined there; N; a policy.  All integer.
  1. volume choice  n[j] = sum_b n_b[j], hs[u][j] = sum_b hs_b[u][j]; (T*, j*) =
     pee_gate_spec.select on the summed table with L = N (pairs with K >= N and K > 0, the
     smallest A / K by exact cross-multiplication, ties to the smaller T, then the smaller j;
     N = 0 gives (1, 0)); G* = GATES[j*].  No feasible pair: status 1, (T*, j*) = (tmax, 15) and
     N := K(tmax, 15) -- the stream's first bits go in, the ungated volume's truncation.
  2. shares         c_b = K_b(T*, j*), P_b = the exclusive prefix sum of c, P_B = the total;
     n_b and off_b by pee_volume_spec's even / fill formulas on these c_b, so that
     sum n_b = N and n_b <= c_b (the argument given there).
  3. per slice      (T_b, j_b) = select on slice b's own table with L = n_b; G_b = GATES[j_b].
     (T*, j*) is feasible for slice b -- K_b(T*, j*) = c_b >= n_b, and n_b > 0 makes it > 0 -- so
     the rule returns a pair with K_b(T_b, j_b) >= n_b: no slice is truncated.  n_b = 0: (1, 0).
  fixed gate g      the tables are the two-class ones (table(..., g_fixed=g)); the rule is
     pee_volume_spec.plan on caps[b][T - 1] = K_b(T, 0), and G_b = g for every slice.
Arithmetic: tmax <= 16, (H//2)(W//2) <= 2^26, B (H//2)(W//2) <= 2^31 - 1, 0 <= N <= 2^31 - 1.
The per-slice cross-products stay below 2^62; the volume choice's do NOT fit 64 bits (the
summed A reaches 2^41, K 2^31) -- Python ints here, 128-bit products on the device.  The scalar
select takes `wrap` to show what a 64-bit comparison would have chosen (the tests' witness).
Row pitch: pee_volume_spec.payload_words.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import pee_gate_spec as G
import pee_volume_spec as V

GATES = G.GATES
POLICIES = V.POLICIES
NMAX = V.NMAX


def K_of(hs, T: int, j: int) -> int:
    """K(T, j) = sum of hs[u][g] over u < T, g <= j."""
    return int(sum(int(hs[u][g]) for u in range(T) for g in range(j + 1)))


def sum_tables(tables):
    n = [sum(int(t[0][j]) for t in tables) for j in range(16)]
    tmax = len(tables[0][1])
    hs = [[sum(int(t[1][u][j]) for t in tables) for j in range(16)] for u in range(tmax)]
    return n, hs


def _check(tables, N, policy):
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {POLICIES}")
    if len(tables) < 1:
        raise ValueError("at least one slice")
    tmax = len(tables[0][1])
    if not 1 <= tmax <= G.TMAX_MAX or any(len(t[0]) != 16 or len(t[1]) != tmax for t in tables):
        raise ValueError("tables must be (n[16], hs[tmax][16]) per slice with one tmax in 1..16")
    if not 0 <= int(N) <= NMAX:
        raise ValueError("N must be in 0..2^31 - 1")
    return tmax


def plan(tables, N: int, policy: str = "even", g_fixed: Optional[int] = None) -> Dict:
    """tables: per slice (n[16], hs[tmax][16]).  Returns status, T (= T*), gate (= G*, or
    g_fixed), total (the bits planned), requested, capacity (= sum of c_b), policy, n[B], t[B],
    g[B] (gate values), off[B + 1] (numpy int64)."""
    tmax = _check(tables, N, policy)
    N = int(N)
    B = len(tables)
    if g_fixed is not None:
        caps = np.array([np.cumsum([int(t[1][u][0]) for u in range(tmax)]) for t in tables], dtype=np.int64)
        p = V.plan(caps, N, policy)
        p["gate"] = int(g_fixed)
        p["g"] = np.full(B, int(g_fixed), np.int64)
        return p
    n_sum, hs_sum = sum_tables(tables)
    requested, status = N, 0
    if N > K_of(hs_sum, tmax, 15):
        status, N = 1, K_of(hs_sum, tmax, 15)
        Ts, js = tmax, 15
    else:
        Ts, js, _k = G.select(n_sum, hs_sum, N)
    K = [np.asarray(G.K_table(t[1])) for t in tables]
    c = [int(K[b][Ts - 1][js]) for b in range(B)]
    P = [0]
    for v in c:
        P.append(P[-1] + v)
    PB = P[B]
    if policy == "even":
        cut = [N * p // PB if PB else 0 for p in P]
        n = [cut[b + 1] - cut[b] for b in range(B)]
    else:
        n = [min(c[b], max(0, N - P[b])) for b in range(B)]
    t, g = [], []
    for b in range(B):
        tb, jb, kb = G.select(tables[b][0], tables[b][1], n[b])
        assert kb >= n[b]
        t.append(tb)
        g.append(GATES[jb])
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return {"status": status, "T": Ts, "gate": GATES[js], "total": N, "requested": requested, "capacity": PB,
            "policy": policy, "n": np.array(n, np.int64), "t": np.array(t, np.int64), "g": np.array(g, np.int64),
            "off": off}


def tables_of(covers: np.ndarray, tmax: int, maxval=None, g_fixed: Optional[int] = None):
    """pee_gate_spec.table of every slice, as lists of Python ints."""
    out = []
    for c in covers:
        n, hs = G.table(c, tmax, maxval, g_fixed)
        out.append(([int(v) for v in n], [[int(v) for v in row] for row in hs]))
    return out


def oracle_embed(covers: np.ndarray, bits: np.ndarray, p: Dict, maxval=None):
    """The gated spec driven by a plan: per slice pee_gate_spec.embed of its share at
    (T_b, G_b).  Returns (stegos, sides)."""
    out = []
    for b, c in enumerate(covers):
        lo, nb = int(p["off"][b]), int(p["n"][b])
        out.append(G.embed(c, bits[lo:lo + nb], int(p["t"][b]), int(p["g"][b]), maxval))
    return np.stack([st for st, _ in out]), [sd for _, sd in out]


def quadrants(img: np.ndarray) -> np.ndarray:
    """The four quadrants of an image as a [4, H/2, W/2] stack (the issue's real-image stacks)."""
    h, w = img.shape[0] // 2, img.shape[1] // 2
    return np.stack([img[:h, :w], img[:h, w:2 * w], img[h:2 * h, :w], img[h:2 * h, w:2 * w]])


# ---------------------------------------------------------------- the tests' stacks
IMAGES = {"pe": 4095, "torax": 255}   # tests/golden/images.npz: name -> maxval
_CACHE: Dict = {}


def stack(source: str):
    """(covers, maxval) of a known-answer source: a pee_volume_spec.BATCHES name (synth.ct12,
    maxval 4095) or "pe" / "torax" (the image's four quadrants)."""
    if source not in _CACHE:
        if source in IMAGES:
            import os
            z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "images.npz"))
            _CACHE[source] = (quadrants(z[source]), IMAGES[source])
        else:
            _CACHE[source] = (V.ct12_batch(source), 4095)
    return _CACHE[source]


def source_tables(source: str, tmax: int, g_fixed: Optional[int] = None):
    """The tables of a known-answer case (computed once per source, tmax and gate).  A source
    "name:k" is the first k slices of "name"; "witnessS" is witness_tables(S)."""
    if ":" in source:
        name, k = source.split(":")
        return source_tables(name, tmax, g_fixed)[:int(k)]
    key = (source, int(tmax), g_fixed)
    if key not in _CACHE:
        if source.startswith("witness"):
            _CACHE[key] = witness_tables(int(source[len("witness"):] or 1), tmax=tmax)
        else:
            covers, maxval = stack(source)
            _CACHE[key] = tables_of(covers, tmax, maxval, g_fixed)
    return _CACHE[key]


# ---------------------------------------------------------------- synthetic tables
def witness_tables(seed: int = 1, B: int = 31, tmax: int = 16, nc: int = 1 << 26) -> List[Tuple[List[int], List[List[int]]]]:
    """B slices of nc candidates each whose counts are spread over all 16 classes and all tmax
    error rows (plus a rest that is never expandable), from a small linear congruential
    generator on Python ints: a stack at the bounds (31 * 2^26 < 2^31), whose summed A K
    products pass 2^64."""
    state = [(seed * 2862933555777941757 + 3037000493) & (2 ** 64 - 1)]

    def rnd(top: int) -> int:
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (state[0] >> 33) % top

    out = []
    for _b in range(B):
        w = [[1 + rnd(1000) for _j in range(16)] for _u in range(tmax + 1)]   # row tmax: the rest
        tot = sum(sum(r) for r in w)
        cells = [[nc * v // tot for v in r] for r in w]
        cells[tmax][15] += nc - sum(sum(r) for r in cells)
        n = [sum(cells[u][j] for u in range(tmax + 1)) for j in range(16)]
        out.append((n, [list(r) for r in cells[:tmax]]))
    return out


# ---------------------------------------------------------------- scalar restatement
def select_scalar(n: Sequence[int], hs: Sequence[Sequence[int]], L: int, wrap: Optional[int] = None):
    """(T, j, K, feasible): the selection rule in plain loops and Python ints.  wrap = 2^64
    reduces the two cross-products modulo 2^64 before they are compared -- what 64-bit unsigned
    arithmetic would do; None compares them exactly."""
    tmax = len(hs)
    L = int(L)
    best = None   # (A, K, T, j)
    Kt = [[0] * 16 for _ in range(tmax + 1)]   # Kt[T][j] = K(T, j), St[T][j] the cost sum, Nt[j] = N(j)
    St = [[0] * 16 for _ in range(tmax + 1)]
    Nt = [0] * 16
    acc = 0
    for j in range(16):
        acc += int(n[j])
        Nt[j] = acc
    for T in range(1, tmax + 1):
        u, row = T - 1, 0
        for j in range(16):
            row += int(hs[u][j])
            Kt[T][j] = Kt[T - 1][j] + row
            St[T][j] = St[T - 1][j] + row * (u * u + (u + 1) * (u + 1))
    for T in range(1, tmax + 1):
        for j in range(16):
            K = Kt[T][j]
            A = 2 * T * T * (Nt[j] - K) + St[T][j]
            if L == 0:
                return T, j, K, True   # the first pair: (1, 0)
            if K >= L and K > 0:
                if best is None:
                    best = (A, K, T, j)
                else:
                    lhs, rhs = A * best[1], best[0] * K
                    if wrap:
                        lhs, rhs = lhs % wrap, rhs % wrap
                    if lhs < rhs:
                        best = (A, K, T, j)
    if best is None:
        K = 0
        for u in range(tmax):
            for g in range(16):
                K += int(hs[u][g])
        return tmax, 15, K, False
    return best[2], best[3], best[1], True


def plan_scalar(tables, N: int, policy: str = "even", g_fixed: Optional[int] = None, wrap: Optional[int] = None) -> Dict:
    """plan() in plain Python loops and ints.  wrap: the volume choice's comparison modulo that
    value (select_scalar); the per-slice choices always compare exactly."""
    tmax = _check(tables, N, policy)
    B = len(tables)
    requested = N = int(N)
    n_sum = [0] * 16
    hs_sum = [[0] * 16 for _ in range(tmax)]
    for nb, hb in tables:
        for j in range(16):
            n_sum[j] += int(nb[j])
            for u in range(tmax):
                hs_sum[u][j] += int(hb[u][j])
    status = 0
    if g_fixed is not None:
        Ts, js, acc = 0, 0, 0
        for T in range(1, tmax + 1):
            acc += hs_sum[T - 1][0]
            if acc >= N:
                Ts = T
                break
        if Ts == 0:
            Ts, status, N = tmax, 1, acc
    else:
        Ts, js, _K, ok = select_scalar(n_sum, hs_sum, N, wrap)
        if not ok:
            status, N = 1, _K
    n, t, g, off = [], [], [], [0]
    PB = 0
    for _nb, hb in tables:
        PB += K_of(hb, Ts, js)
    Pb = 0
    for nb_tab, hb in tables:
        c = K_of(hb, Ts, js)
        if policy == "even":
            share = (N * (Pb + c) // PB - N * Pb // PB) if PB else 0
        else:
            share = min(c, max(0, N - Pb))
        Pb += c
        if g_fixed is not None:
            tb, acc = 0, 0
            for T in range(1, tmax + 1):
                acc += int(hb[T - 1][0])
                if acc >= share:
                    tb = T
                    break
            assert tb > 0
            gb = int(g_fixed)
        else:
            tb, jb, kb, ok = select_scalar(nb_tab, hb, share)
            assert ok and kb >= share
            gb = GATES[jb]
        n.append(share)
        t.append(tb)
        g.append(gb)
        off.append(off[-1] + share)
    return {"status": status, "T": Ts, "gate": int(g_fixed) if g_fixed is not None else GATES[js], "total": N,
            "requested": requested, "capacity": PB, "policy": policy, "n": n, "t": t, "g": g, "off": off}

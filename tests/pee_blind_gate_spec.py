"""Specification of gated blind MED-PEE: (T, gate) chosen per slice, the gate carried in the header.
TEST INFRASTRUCTURE ONLY: the kernels behind include/codec_tcc_blind_gate.h are checked bit-exact
against plan() / choose() / embed() / decode() / capacity_curve(), and those against the scalar
restatement tests/pee_blind_gate_scalar.py.

  gate      G = GATES[j], j in 0..15 (tests/pee_gate_spec.py's ladder); a candidate is ACTIVE iff its
            roughness D = max(W, N, NW) - min(W, N, NW) <= G.  D reads pixels of even rows or
            columns, which scheme 1 never modifies, and for a candidate above the reserved rows they
            lie above those rows too: the decoder computes the same D
  plan      tests/pee_blind_spec.py's plan at (T, G) with gated counts: cap_i counts the candidates
            through row i that are active, expandable and safe; uns_i those that are active and
            unsafe (an inactive candidate is never modified and needs no map entry).  i*, E =
            uns_{i*}, n_side = 192 + 32 E, r, the rectangle, statuses 1 and 2 and the capacity
            (the maximum of cap_i - 192 - 32 uns_i over the rows with i < hc - r_i and
            uns_i <= max_entries) are that plan's
  embed     the ROI embed of tests/pee_roi_spec.py at (T, G, the rectangle) on displaced || user:
            status 0, `end` in a row <= i*, at most E map bits
  rule      over the pairs (T, j), T in 1..tmax, j in 0..15: the smallest T for which some j has a
            plan of status 0, and at that T the smallest such j.  Nothing is assumed monotone in T or
            j.  A fixed T (in 1..tmax) or a fixed gate (a ladder value) leaves the rule the other one
  refusal   no pair qualifies: the slice is copied through with no header; its info is the plan's at
            (tmax, j = 15), or at the fixed values; its chosen T is 0 and its gate -1
  header    pee_blind_spec's six words; flag bit 3 (FLAG_GATED) marks a gated slice, whose flag bits
            4-7 hold j (also at j = 15).  Without bit 3, bits 4-7 are 0
  decode    one decoder for gated and ungated slices: G = GATES[j] with bit 3, no gate without
  capacity  curve[T - 1][j] = plan(cover, 0, T, j)["capacity"]
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle.pee_cpu import _grids, classify, med

try:   # with tests/ on the path (the suite, the golden generator) or as tests.pee_blind_gate_spec
    import pee_blind_spec as BS
    import pee_roi_spec as RS
except ImportError:   # pragma: no cover
    from tests import pee_blind_spec as BS
    from tests import pee_roi_spec as RS

GATES = RS.GS.GATES
FLAG_CRC = BS.FLAG_CRC
FLAG_GATED = 8
FLAG_J_SHIFT = 4
TMAX = 16
HDR_BITS = BS.HDR_BITS


def gate_index(G: int) -> int:
    if int(G) not in GATES:
        raise ValueError(f"the gate must be one of the ladder {GATES}")
    return GATES.index(int(G))


def row_counts(cover: np.ndarray, T: int, G: int, maxval: int) -> Tuple[np.ndarray, np.ndarray]:
    """(es[hc], uns[hc]) over the ACTIVE candidates of each candidate row."""
    x, a, b, c = _grids(cover)
    _e, expand, _right, safe = classify(x, med(a, b, c), T, maxval)
    act = RS.GS.roughness(a, b, c) <= G
    return (expand & safe & act).sum(axis=1).astype(np.int64), (~safe & act).sum(axis=1).astype(np.int64)


def plan_rows(es, uns, n_user: int, H: int, W: int, max_entries: int) -> Dict:
    """pee_blind_spec.plan's rule on one pair's row counts."""
    hc = H // 2
    cap, un = np.cumsum(es), np.cumsum(uns)
    room = cap - HDR_BITS - 32 * un
    rr = -(-(HDR_BITS + 32 * un) // (2 * W))
    valid = (np.arange(hc) < hc - rr) & (un <= max_entries)
    capacity = int(room[valid].max()) if valid.any() else -1
    out = {"status": 0, "n_user": int(n_user), "E": 0, "n_side": 0, "i_star": -1, "r": 0, "rect": (0, 0, 0, 0),
           "capacity": max(capacity, -1)}
    hit = np.flatnonzero(room >= n_user)
    if hit.size == 0:
        out["status"] = 1
        return out
    i = int(hit[0])
    E = int(un[i])
    n_side = HDR_BITS + 32 * E
    r, rect = BS.region(H, W, n_side)
    out.update(E=E, i_star=i)
    if i >= hc - r:
        out["status"] = 1
    elif E > max_entries:
        out["status"] = 2
    else:
        out.update(n_side=n_side, r=r, rect=rect)
    return out


def plan(cover: np.ndarray, n_user: int, T: int, j: int, maxval: Optional[int] = None, max_entries: int = 256) -> Dict:
    H, W = cover.shape
    es, uns = row_counts(cover, T, GATES[j], BS._maxval(cover, maxval))
    return plan_rows(es, uns, n_user, H, W, max_entries)


def _pairs(tmax: int, T, gate) -> Tuple[List[int], List[int]]:
    if not 1 <= int(tmax) <= TMAX:
        raise ValueError(f"tmax in 1..{TMAX}")
    if T is not None and not 1 <= int(T) <= int(tmax):
        raise ValueError("a fixed T lies in 1..tmax")
    return ([int(T)] if T is not None else list(range(1, int(tmax) + 1)),
            [gate_index(gate)] if gate is not None else list(range(16)))


def tables(cover: np.ndarray, ts, maxval: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(es, uns) as int64 [len(ts)][16][hc]: row_counts at every (T in ts, GATES[j]), from one
    classification per T and one class per candidate (the first j with D <= GATES[j])."""
    maxval = BS._maxval(cover, maxval)
    x, a, b, c = _grids(cover)
    p = med(a, b, c)
    hc, wc = x.shape
    key = (np.repeat(np.arange(hc), wc) * 16 + RS.GS.gate_class(RS.GS.roughness(a, b, c)).ravel()).astype(np.int64)
    es, uns = np.zeros((len(ts), 16, hc), np.int64), np.zeros((len(ts), 16, hc), np.int64)
    for k, T in enumerate(ts):
        _e, expand, _right, safe = classify(x, p, int(T), maxval)
        for out, m in ((es, expand & safe), (uns, ~safe)):
            n = np.bincount(key[m.ravel()], minlength=hc * 16).reshape(hc, 16)
            out[k] = np.cumsum(n, axis=1).T
    return es, uns


def choose(cover: np.ndarray, n_user: int, tmax: int, maxval: Optional[int] = None, max_entries: int = 256, T=None,
           gate=None) -> Tuple[int, int, Dict]:
    """(T*, j*, plan there), or (0, -1, the plan at the last T and the last j considered)."""
    ts, js = _pairs(tmax, T, gate)
    H, W = cover.shape
    es, uns = tables(cover, ts, maxval)
    p = None
    for k, t in enumerate(ts):
        for j in js:
            p = plan_rows(es[k][j], uns[k][j], n_user, H, W, max_entries)
            if p["status"] == 0:
                return t, j, p
    return 0, -1, p


def capacity_curve(cover: np.ndarray, tmax: int, maxval: Optional[int] = None, max_entries: int = 256) -> List[List[int]]:
    ts, js = _pairs(tmax, None, None)
    H, W = cover.shape
    es, uns = tables(cover, ts, maxval)
    return [[plan_rows(es[k][j], uns[k][j], 0, H, W, max_entries)["capacity"] for j in js] for k in range(len(ts))]


def embed_at(cover: np.ndarray, bits, T: int, j: int, maxval: Optional[int] = None, checksum: bool = False,
             max_entries: int = 256) -> Tuple[np.ndarray, Tuple[int, ...], Dict]:
    """(stego, info, plan) at one pair.  A refused slice: the cover, (status, n_user, E, 0, -1, 0)."""
    if cover.dtype not in (np.uint8, np.uint16) or cover.ndim != 2:
        raise ValueError("cover must be a 2-D uint8/uint16 image")
    H, W = cover.shape
    if H > BS.MAX_DIM or W > BS.MAX_DIM:
        raise ValueError("blind MED-PEE takes H, W <= 65535")
    maxval = BS._maxval(cover, maxval)
    if not 1 <= T <= 64 or not 1 <= maxval <= 65535 or not 0 <= j <= 15:
        raise ValueError("T in 1..64, maxval in 1..65535, j in 0..15")
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    p = plan(cover, bits.size, T, j, maxval, max_entries)
    if p["status"]:
        return cover.copy(), (p["status"], bits.size, p["E"], 0, -1, 0), p
    n_side, E = p["n_side"], p["E"]
    idx = BS.side_index(H, W, n_side)
    displaced = (cover.ravel()[idx] & 1).astype(np.uint8)
    stego, side = RS.embed(cover, np.concatenate([displaced, bits]), T, GATES[j], p["rect"], maxval)
    assert side["status"] == 0 and side["lm_count"] <= E
    assert side["end"] < (p["i_star"] + 1) * (W // 2)
    y0 = p["rect"][0]
    assert np.array_equal(stego[y0:], cover[y0:])
    flags = (FLAG_CRC if checksum else 0) | FLAG_GATED | (j << FLAG_J_SHIFT)
    words = BS.header(T, flags, maxval, bits.size, E, side["end"], BS.cover_crc(cover) if checksum else 0,
                      np.flatnonzero(side["lm"]))
    flat = stego.ravel()   # a view: stego is contiguous
    flat[idx] = (flat[idx] & ~np.asarray(1, stego.dtype)) | BS.words_to_bits(words).astype(stego.dtype)
    return stego, (0, bits.size, E, n_side, side["end"], y0), p


def embed(cover: np.ndarray, bits, tmax: int, maxval: Optional[int] = None, checksum: bool = False,
          max_entries: int = 256, T=None, gate=None) -> Tuple[np.ndarray, Tuple[int, ...], int, int, Dict]:
    """(stego, info, T*, G*, plan): embed_at the chosen pair; refused: T* = 0, G* = -1, the cover."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    ts, js = _pairs(tmax, T, gate)
    t, j, _p = choose(cover, bits.size, tmax, maxval, max_entries, T, gate)
    stego, info, p = embed_at(cover, bits, t if t else ts[-1], j if t else js[-1], maxval, checksum, max_entries)
    assert (info[0] == 0) == (t != 0)
    return stego, info, t, (GATES[j] if t else -1), p


def split_flags(flags: int) -> Tuple[int, int]:
    """(the flags pee_blind_spec knows, G or BS.GATE_NONE); ValueError for bits 4-7 without bit 3."""
    if not flags & FLAG_GATED:
        if flags & 0xF0:
            raise ValueError(f"flags = {flags:#x} (bits 4-7 hold a gate only beside bit 3)")
        return flags, BS.GATE_NONE
    return flags & ~(FLAG_GATED | 0xF0), GATES[(flags >> FLAG_J_SHIFT) & 15]


def decode(stego: np.ndarray, verify: bool = True) -> Tuple[np.ndarray, np.ndarray, Dict]:
    """(user bits, cover, header with "G"): gated and ungated slices alike."""
    H, W = stego.shape
    if H * W < HDR_BITS:
        raise ValueError("the slice cannot hold a header")
    words = [int(v) for v in BS.read_words(stego, 0, BS.HDR_WORDS)]
    flags = (words[1] >> 8) & 0xFF
    rest, G = split_flags(flags) if words[0] == BS.MAGIC else (flags, BS.GATE_NONE)
    words[1] = (words[1] & ~0xFF00) | (rest << 8)
    h = BS.check_header(words, H, W, int(np.iinfo(stego.dtype).max))
    h.update(flags=flags, G=G)
    nc = (H // 2) * (W // 2)
    ent = BS.read_words(stego, BS.HDR_WORDS, h["E"]) if h["E"] else np.zeros(0, np.uint64)
    lm = np.zeros(h["end"] + 1, bool)
    for v in ent:
        if int(v) != BS.NO_ENTRY and int(v) <= h["end"] and int(v) < nc:
            lm[int(v)] = True
    got, cover = RS.extract(stego, {"T": h["T"], "G": G, "end": h["end"], "L": h["L"], "lm": lm, "roi": h["rect"]})
    if got.size != h["L"]:
        raise ValueError(f"the slice yields {got.size} bits, its header states {h['L']}")
    idx = BS.side_index(H, W, h["n_side"])
    flat = cover.ravel()
    flat[idx] = (flat[idx] & ~np.asarray(1, cover.dtype)) | got[:h["n_side"]].astype(cover.dtype)
    if verify and (flags & FLAG_CRC) and BS.cover_crc(cover) != h["crc"]:
        raise ValueError("the restored cover fails the header's CRC")
    return got[h["n_side"]:], cover, h

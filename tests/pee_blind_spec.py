"""Specification of blind MED-PEE (scheme 1, fixed T): a stego that carries its own location map
and record, so that it decodes with nothing beside it.  TEST INFRASTRUCTURE ONLY: the HIP kernels
of codec_tcc_amd/csrc/codec_blind.hip are checked bit-exact against plan() / embed() / decode(),
and those against the scalar restatement tests/pee_blind_scalar.py.

  notation   hc = H // 2, wc = W // 2, nc = hc * wc; candidates in raster order; classify is
             oracle/pee_cpu.py's at (T, maxval) on the COVER
  side bits  n_side = 192 + 32 E.  Side bit i is bit 0 of the pixel with flat index H W - 1 - i
             (the stream runs backwards from the last pixel); words are 32 bits, LSB first: side
             bit 32 k + j is bit j of word k
  words      0 magic 0x4D504231; 1 T (bits 0-7) | flags (bits 8-15; bit 0: word 5 holds the
             cover's CRC) | maxval (bits 16-31); 2 n_user; 3 E; 4 end (0xFFFFFFFF for -1);
             5 CRC-32 of the cover slice's little-endian bytes (zlib), or 0; 6 .. 5 + E the
             ascending candidate indices of the location map's set bits up to `end`, then
             0xFFFFFFFF padding
  plan       from the cover alone: cap_i / uns_i = the cumulative counts, through candidate row i,
             of expandable-and-safe / unsafe candidates; i* = the first row with
             cap_i >= n_user + 192 + 32 uns_i; E = uns_{i*}; r = ceil(n_side / (2 W)); the
             reserved region is the rectangle (2 (hc - r), 0, H, W)
  refusals   status 1 (capacity): no row qualifies, or i* >= hc - r; then status 2: E > max_entries.
             A refused slice is copied through unchanged and carries no header; its info is
             (status, n_user, E, 0, -1, 0) with E = 0 when no row qualified
  capacity   the largest n_user with status 0, -1 when not even n_user = 0 fits
  embed      PEE payload = the n_side displaced cover LSBs (displaced[i] = bit 0 of pixel
             H W - 1 - i), then the user bits; embedded by the ROI embed of tests/pee_roi_spec.py at
             (T, no gate, the rectangle): status 0, `end` in a row <= i*, at most E map bits; the
             side words then replace the LSBs of the first n_side reverse-raster pixels of the stego
  info       (status, n_user, E, n_side, end, region row = 2 (hc - r))
  decode     words 0-5; refuse a bad magic, T, maxval, end, E or n_side (ValueError); rebuild the
             rectangle from n_side and the map from the entries; ROI extract with L = n_side +
             n_user; the first n_side extracted bits go back into the LSBs, the rest is the payload
"""
from __future__ import annotations

import zlib
from typing import Dict, Optional, Tuple

import numpy as np

from oracle.pee_cpu import _grids, classify, med

try:   # with tests/ on the path (the suite, the golden generator) or as tests.pee_blind_spec
    import pee_roi_spec as RS
except ImportError:   # pragma: no cover
    from tests import pee_roi_spec as RS

MAGIC = 0x4D504231
HDR_WORDS = 6
HDR_BITS = 32 * HDR_WORDS
NO_ENTRY = 0xFFFFFFFF
FLAG_CRC = 1
GATE_NONE = 65535
MAX_DIM = 65535


def _maxval(cover: np.ndarray, maxval: Optional[int]) -> int:
    return int(np.iinfo(cover.dtype).max) if maxval is None else int(maxval)


def cover_crc(cover: np.ndarray) -> int:
    return zlib.crc32(np.ascontiguousarray(cover).astype(cover.dtype.newbyteorder("<"), copy=False).tobytes()) & 0xFFFFFFFF


def row_counts(cover: np.ndarray, T: int, maxval: int) -> Tuple[np.ndarray, np.ndarray]:
    """(es[hc], uns[hc]): per candidate row, the expandable-and-safe and the unsafe candidates."""
    x, a, b, c = _grids(cover)
    _e, expand, _right, safe = classify(x, med(a, b, c), T, maxval)
    return (expand & safe).sum(axis=1).astype(np.int64), (~safe).sum(axis=1).astype(np.int64)


def region(H: int, W: int, n_side: int) -> Tuple[int, Tuple[int, int, int, int]]:
    """(r, rectangle) of a slice that carries n_side side bits."""
    r = -(-n_side // (2 * W))
    return r, (2 * (H // 2 - r), 0, H, W)


def plan(cover: np.ndarray, n_user: int, T: int, maxval: Optional[int] = None, max_entries: int = 256) -> Dict:
    H, W = cover.shape
    hc = H // 2
    maxval = _maxval(cover, maxval)
    es, uns = row_counts(cover, T, maxval)
    cap, un = np.cumsum(es), np.cumsum(uns)
    room = cap - HDR_BITS - 32 * un                       # user bits that fit when the payload ends in row i
    rr = -(-(HDR_BITS + 32 * un) // (2 * W))
    valid = (np.arange(hc) < hc - rr) & (un <= max_entries)   # a prefix of the rows: un and rr never fall
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
    r, rect = region(H, W, n_side)
    out.update(E=E, i_star=i)
    if i >= hc - r:
        out["status"] = 1
    elif E > max_entries:
        out["status"] = 2
    else:
        out.update(n_side=n_side, r=r, rect=rect)
    return out


def side_index(H: int, W: int, n_side: int) -> np.ndarray:
    """Flat pixel index of side bit i, i < n_side."""
    return H * W - 1 - np.arange(n_side)


def words_to_bits(words) -> np.ndarray:
    w = np.asarray(words, dtype=np.uint64)
    return ((w[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).ravel()


def bits_to_words(bits) -> np.ndarray:
    b = np.asarray(bits, dtype=np.uint64).reshape(-1, 32)
    return (b << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)


def header(T: int, flags: int, maxval: int, n_user: int, E: int, end: int, crc: int, entries) -> np.ndarray:
    ent = [int(v) for v in entries]
    assert len(ent) <= E
    return np.array([MAGIC, T | (flags << 8) | (maxval << 16), n_user, E, end & 0xFFFFFFFF, crc] + ent +
                    [NO_ENTRY] * (E - len(ent)), dtype=np.uint64)


def embed(cover: np.ndarray, bits, T: int, maxval: Optional[int] = None, checksum: bool = False,
          max_entries: int = 256) -> Tuple[np.ndarray, Tuple[int, ...], Dict]:
    """(stego, info, plan).  A refused slice: the cover, (status, n_user, E, 0, -1, 0)."""
    if cover.dtype not in (np.uint8, np.uint16) or cover.ndim != 2:
        raise ValueError("cover must be a 2-D uint8/uint16 image")
    H, W = cover.shape
    if H > MAX_DIM or W > MAX_DIM:
        raise ValueError("blind MED-PEE takes H, W <= 65535")
    maxval = _maxval(cover, maxval)
    if not 1 <= T <= 64 or not 1 <= maxval <= 65535:
        raise ValueError("T in 1..64 and maxval in 1..65535")
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    p = plan(cover, bits.size, T, maxval, max_entries)
    if p["status"]:
        return cover.copy(), (p["status"], bits.size, p["E"], 0, -1, 0), p
    n_side, E = p["n_side"], p["E"]
    idx = side_index(H, W, n_side)
    displaced = (cover.ravel()[idx] & 1).astype(np.uint8)
    stego, side = RS.embed(cover, np.concatenate([displaced, bits]), T, GATE_NONE, p["rect"], maxval)
    assert side["status"] == 0 and side["lm_count"] <= E
    assert side["end"] < (p["i_star"] + 1) * (W // 2)
    y0 = p["rect"][0]
    assert np.array_equal(stego[y0:], cover[y0:])
    words = header(T, FLAG_CRC if checksum else 0, maxval, bits.size, E, side["end"],
                   cover_crc(cover) if checksum else 0, np.flatnonzero(side["lm"]))
    flat = stego.ravel()   # a view: stego is contiguous
    flat[idx] = (flat[idx] & ~np.asarray(1, stego.dtype)) | words_to_bits(words).astype(stego.dtype)
    return stego, (0, bits.size, E, n_side, side["end"], y0), p


def read_words(stego: np.ndarray, first: int, count: int) -> np.ndarray:
    """Side words first .. first + count - 1 of a slice (it must hold that many side bits)."""
    H, W = stego.shape
    idx = H * W - 1 - np.arange(32 * first, 32 * (first + count))
    return bits_to_words(stego.ravel()[idx] & 1)


def check_header(words, H: int, W: int, vmax: int) -> Dict:
    """The decoder's refusals, as ValueError naming the field; the header as a dict."""
    w = [int(v) for v in words[:HDR_WORDS]]
    nc = (H // 2) * (W // 2)
    if w[0] != MAGIC:
        raise ValueError(f"magic = {w[0]:#010x} (no blind MED-PEE header: {MAGIC:#010x})")
    T, flags, maxval = w[1] & 0xFF, (w[1] >> 8) & 0xFF, w[1] >> 16
    if not 1 <= T <= 64:
        raise ValueError(f"T = {T} (1..64)")
    if flags & ~FLAG_CRC:
        raise ValueError(f"flags = {flags:#x} (bit 0 alone is defined)")
    if not 1 <= maxval <= vmax:
        raise ValueError(f"maxval = {maxval} (1..{vmax})")
    n_user, E = w[2], w[3]
    end = -1 if w[4] == NO_ENTRY else w[4]
    if end >= nc:
        raise ValueError(f"end = {end} (the slice has {nc} candidates)")
    n_side = HDR_BITS + 32 * E
    if E > nc or n_side > H * W:
        raise ValueError(f"E = {E} (the slice cannot hold {n_side} side bits)")
    r, rect = region(H, W, n_side)
    if r > H // 2:
        raise ValueError(f"n_side = {n_side} (more than the slice's candidate rows hold)")
    if end >= (H // 2 - r) * (W // 2):
        raise ValueError(f"end = {end} (inside the reserved region, which starts at candidate row {H // 2 - r})")
    L = n_side + n_user
    if L > end + 1:
        raise ValueError(f"n_user = {n_user} ({L} bits cannot lie in candidates 0..{end})")
    return {"T": T, "flags": flags, "maxval": maxval, "n_user": n_user, "E": E, "end": end, "crc": w[5],
            "n_side": n_side, "rect": rect, "L": L}


def decode(stego: np.ndarray, verify: bool = True) -> Tuple[np.ndarray, np.ndarray, Dict]:
    """(user bits, cover, header).  ValueError for a slice without a valid header or whose restored
    cover fails the CRC the header carries."""
    H, W = stego.shape
    if H * W < HDR_BITS:
        raise ValueError("the slice cannot hold a header")
    h = check_header(read_words(stego, 0, HDR_WORDS), H, W, int(np.iinfo(stego.dtype).max))
    nc = (H // 2) * (W // 2)
    ent = read_words(stego, HDR_WORDS, h["E"]) if h["E"] else np.zeros(0, np.uint64)
    lm = np.zeros(h["end"] + 1, bool)
    for v in ent:
        if int(v) != NO_ENTRY and int(v) <= h["end"] and int(v) < nc:
            lm[int(v)] = True
    side = {"T": h["T"], "G": GATE_NONE, "end": h["end"], "L": h["L"], "lm": lm, "roi": h["rect"]}
    got, cover = RS.extract(stego, side)
    if got.size != h["L"]:
        raise ValueError(f"the slice yields {got.size} bits, its header states {h['L']}")
    idx = side_index(H, W, h["n_side"])
    flat = cover.ravel()
    flat[idx] = (flat[idx] & ~np.asarray(1, cover.dtype)) | got[:h["n_side"]].astype(cover.dtype)
    if verify and (h["flags"] & FLAG_CRC) and cover_crc(cover) != h["crc"]:
        raise ValueError("the restored cover fails the header's CRC")
    return got[h["n_side"]:], cover, h


def capacity(cover: np.ndarray, T: int, maxval: Optional[int] = None, max_entries: int = 256) -> int:
    return plan(cover, 0, T, maxval, max_entries)["capacity"]

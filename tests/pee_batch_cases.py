"""Batches at which codec_pee.hip's dispatch changes route, for every MED-PEE feature (test
infrastructure; seeded, no files, no GPU but for ncu()).  tests/test_pee_batch_dispatch.py runs
them on the GPU with no knob set; tests/test_pee_batch_cases_host.py checks the conditions below on
the specifications alone.

Batch sizes (batches(ncu); on the MI355X, 256 CUs: 255, 256, 265, 436)
  below       ncu - 1: the grouped look-back, last group ragged
  fills       ncu: chip-filling (pee_fills_chip), the slice-serial kernels where a call has them
  ragged      ncu + 9: B / (2 ncu) < 0.85, the look-back again; ceil(B / 8) lanes, the last holding
              one slice, and a partial last group of 32
  two_rounds  ceil(0.85 * 2 ncu): chip-filling with more workgroups than CUs

Slices are 67 x 264 (tests/test_pee_launch_variants.py's BASE): W % 8 == 0 admits the vector
routes, 33 x 33 = 1089 items of 8 pixels x 2 rows are two 1024-item chunks, the second ragged (it
starts at candidate 4096 = SECOND_CHUNK of the 4356), and the odd H exercises the last-row copy.

Every slice of a family is a function of its index b alone, so a batch of B slices is the first B
of the family and a specification result is computed once for all batch sizes (the keyed
families, whose nonce holds the global index 2^31 - B + b, are a function of (b, B)).
  covers      synth.ct12(67, 264, SEED + b) at maxval 4095, the u8 generator at 255; the blind
              families: pee_blind_cases.smooth, every fifth slice planted(3 or 4 pixels), every
              eleventh with pee_blind_auto_cases' bright block, and a dozen pixels of the lower half
              nudged by one, seeded by b
  lengths     cycle with period 7 (coprime to the lanes' 8 and the groups' 32) over the slice's own
              capacity: LENGTHS below; the T = "auto" families over its capacity curve: AUTO_LENGTHS
  T, G, rect  cycle with period 5 (coprime to 7, 8, 32): T_CYCLE, G_CYCLE, rect()
No two slices of a batch have equal specification stego, so a per-slice array indexed by anything
but the slice cannot pass; each batch holds an empty payload, one that ends in the second chunk and
one that overflows (blind: is refused).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import aead_spec as AES
import pee_blind_auto_spec as BAS
import pee_blind_cases as CS
import pee_blind_keyed_spec as BKS
import pee_blind_spec as BS
import pee_gate_spec as G
import pee_gvol_spec as GV
import pee_roi_spec as R
import pee_volume_spec as V
from codec_tcc_amd import synth
from oracle import pee_cpu as P

H, W = 67, 264
NC = (H // 2) * (W // 2)
SECOND_CHUNK = 4 * 1024          # the first candidate of the second 1024-item chunk (4 candidates an item)
SEED = 7000
MAX_NCU = 1024
NO_GATE = 65535
T_FIXED = 2
TMAX = 8                         # the capacity-controlled families (scheme 1, scheme 2, blind)
GATE_TMAX = 16                   # gate="auto"
T_CYCLE = (2, 1, 3, 5, 2)
G_CYCLE = (24, 12, 48, 24, NO_GATE)
BLIND_T, BLIND_ME = 4, 16        # max_entries 16 admits the bright block's 13 unsafe candidates
KEY = bytes(range(1, 33))
NONCE = bytes(range(0xA0, 0xA8))
NONCE_2 = bytes(range(0xC0, 0xC8))
TILE = 16
SATURATED = 40                   # the volume families' slice without capacity
GRID_SHAPE = (258, 512)          # the persistent-grid case: 129 x 64 items = 9 chunks a slice


def ncu() -> int:
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def batches(ncu: int) -> dict:
    return {"below": ncu - 1, "fills": ncu, "ragged": ncu + 9, "two_rounds": math.ceil(0.85 * 2 * ncu)}


def fills_chip(B: int, ncu: int) -> bool:
    """pee_fills_chip of codec_pee.hip"""
    return B >= ncu and B / (-(-B // ncu) * ncu) >= 0.85


def maxval(dtype) -> int:
    return 4095 if np.dtype(dtype) == np.uint16 else 255


def payload(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(3 * SEED + seed).integers(0, 2, max(int(n), 0)).astype(np.uint8)


def length(b: int, cap: int, fit: bool = False) -> int:
    """LENGTHS: nothing; half; `end` in the last chunk; 41 bits too many (fit: the capacity itself);
    one bit; the capacity; a third"""
    cap = max(int(cap), 0)
    return (0, cap // 2, max(cap - 3, 0), cap if fit else cap + 41, min(1, cap) if fit else 1, cap, cap // 3)[b % 7]


def auto_length(b: int, curve, fit: bool = False) -> int:
    """AUTO_LENGTHS over the capacities at T = 1..tmax: nothing; inside T = 1; just past T = 1; between
    T = 3 and 4; `end` in the last chunk at tmax; 60 bits beyond every T (fit: the largest); one bit"""
    c = [max(int(v), 0) for v in curve]
    top = max(c)
    return (0, c[0] // 2, min(c[0] + 7, top), (c[2] + c[3]) // 2, max(top - 3, 0), top if fit else top + 60,
            min(1, top) if fit else 1)[b % 7]


def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cover(dtype: str, b: int) -> np.ndarray:
    return _frozen(synth.GENERATORS["ct12" if dtype == "uint16" else "u8"](H, W, SEED + b))


def covers(dtype: str, B: int) -> np.ndarray:
    return np.stack([cover(dtype, b) for b in range(B)])


def rect(b: int):
    """none; central with odd edges; vertical edges inside an 8-column item; the whole slice; an empty
    one (x0 == x1: it normalises to none)"""
    return ((0, 0, 0, 0), (17, 67, 51, 199), (1, 11, 45, 29), (0, 0, H, W), (20, 30, 20, 90))[b % 5]


# ------------------------------------------------------------------ scheme 1 and 2, fixed T and "auto"
@functools.lru_cache(maxsize=None)
def fixed(dtype: str, b: int, fit: bool = False):
    """(cover, bits, stego, side) at T_FIXED; fit: no slice overflows (decode() refuses one)"""
    c, mv = cover(dtype, b), maxval(dtype)
    bits = payload(length(b, P.capacity(c, T_FIXED, mv), fit), b)
    st, side = P.pee_embed(c, bits, T_FIXED, mv, truncate=True)
    return c, bits, _frozen(st), side


@functools.lru_cache(maxsize=None)
def auto(dtype: str, b: int):
    """(cover, bits, T, stego, side): pee_cpu.select_T, then the truncating embed at that T"""
    c, mv = cover(dtype, b), maxval(dtype)
    bits = payload(auto_length(b, P.capacity_curve(c, TMAX, mv)), 1000 + b)
    T = P.select_T(c, len(bits), TMAX, mv)
    st, side = P.pee_embed(c, bits, T, mv, truncate=True)
    return c, bits, T, _frozen(st), side


@functools.lru_cache(maxsize=None)
def _multi_capacity(dtype: str, b: int, T: int) -> int:
    c = cover(dtype, b)
    return P.pee_embed_multi(c, np.zeros(c.size, np.uint8), T, maxval=maxval(dtype))[1]["L"]


@functools.lru_cache(maxsize=None)
def scheme2(dtype: str, b: int):
    """(cover, bits, stego, side) of the four passes at T_FIXED"""
    c = cover(dtype, b)
    bits = payload(length(b, _multi_capacity(dtype, b, T_FIXED)), 2000 + b)
    st, side = P.pee_embed_multi(c, bits, T_FIXED, maxval=maxval(dtype))
    return c, bits, _frozen(st), side


@functools.lru_cache(maxsize=None)
def scheme2_auto(dtype: str, b: int):
    """(cover, bits, T, stego, side): the first T in 1..TMAX whose four passes place every bit, else
    TMAX truncated (tests/test_pee2_auto.py's spec_auto)"""
    c, mv = cover(dtype, b), maxval(dtype)
    bits = payload(auto_length(b, [_multi_capacity(dtype, b, T) for T in (1, 2, 3, 4, TMAX)]), 3000 + b)
    for T in range(1, TMAX + 1):
        st, side = P.pee_embed_multi(c, bits, T, maxval=mv)
        if side["status"] == 0:
            break
    return c, bits, T, _frozen(st), side


# ------------------------------------------------------------------ gate and ROI
@functools.lru_cache(maxsize=None)
def gate(dtype: str, b: int):
    """(cover, bits, T, G, stego, side) at the slice's (T, G) of the cycles; uint8: G of the u8
    generator's scale (four times the cycle's, the open gate as it is)"""
    c, mv = cover(dtype, b), maxval(dtype)
    T, g = T_CYCLE[b % 5], G_CYCLE[b % 5]
    if dtype == "uint8" and g != NO_GATE:
        g *= 4
    bits = payload(length(b, G.embed(c, [], T, g, mv)[1]["capacity"]), 4000 + b)
    st, side = G.embed(c, bits, T, g, mv)
    return c, bits, T, g, _frozen(st), side


@functools.lru_cache(maxsize=None)
def gate_auto(b: int):
    """(cover, bits, T, G, stego, side): gate="auto", T="auto" -- pee_gate_spec's table and select at
    GATE_TMAX; the lengths cycle over the open gate's curve"""
    c, mv = cover("uint16", b), 4095
    n, hs = G.table(c, GATE_TMAX, mv)
    K = G.K_table(hs)
    bits = payload(auto_length(b, [int(K[T - 1][15]) for T in (1, 2, 3, 4, GATE_TMAX)]), 5000 + b)
    T, j, _k = G.select(n, hs, len(bits), 0)
    st, side = G.embed(c, bits, T, G.GATES[j], mv)
    return c, bits, T, G.GATES[j], _frozen(st), side


@functools.lru_cache(maxsize=None)
def roi(b: int):
    """(cover, bits, T, G, rect, stego, side); the rectangles' period is 5 as T's and G's, so they are
    assigned by b // 5 to meet every (T, G)"""
    c, mv = cover("uint16", b), 4095
    T, g, rc = T_CYCLE[b % 5], G_CYCLE[b % 5], rect(b // 5 + b)
    bits = payload(length(b, R.embed(c, [], T, g, rc, mv)[1]["capacity"]), 6000 + b)
    st, side = R.embed(c, bits, T, g, rc, mv)
    return c, bits, T, g, rc, _frozen(st), side


def bbox_mask(b: int) -> np.ndarray:
    """A mask for roi.roi_bbox: slice b has the pixels of its rect() set (an empty mask for none)"""
    y0, x0, y1, x1 = R.normalize(rect(b), H, W)
    m = np.zeros((H, W), np.uint16)
    m[y0:y1, x0:x1] = 1 + b
    return m


# ------------------------------------------------------------------ keyed (PeeCodec.embed(key=))
def index0(B: int) -> int:
    return 2 ** 31 - B


def _row(bits: np.ndarray):
    return BKS._row(np.asarray(bits, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def keyed(b: int, B: int, fit: bool = False):
    """(cover, bits, ciphertext row, tag, stego, side): the plain embed of aead_spec's ciphertext"""
    c, bits, _st, _side = fixed("uint16", b, fit)
    g, n = index0(B) + b, len(bits)
    ct = AES.crypt_row(KEY, NONCE, g, _row(bits), n)
    tag = AES.tag(KEY, NONCE, g, c.tobytes(), ct, n)
    ct_bits = np.unpackbits(np.frombuffer(AES.row_bytes(ct, n), dtype=np.uint8), bitorder="little")[:n]
    st, side = P.pee_embed(c, ct_bits, T_FIXED, 4095, truncate=True)
    return c, bits, ct, tag, _frozen(st), side


# ------------------------------------------------------------------ volumes
@functools.lru_cache(maxsize=None)
def volume_covers(B: int) -> np.ndarray:
    """ct12 slices; slice SATURATED is all 4095 and holds nothing, so every plan gives it no bits"""
    c = covers("uint16", B)
    c[SATURATED] = 4095
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def volume_bits(B: int, gated: bool = False) -> np.ndarray:
    """The stream: halfway between the stack's capacities at T = 2 and T = 3 (so T* = 3 and the
    slices' own T differ); "fill" then leaves the last slices empty.  gated: half the stack's
    capacity at T = 1, which gate="auto" spreads over the (T, G) ladder"""
    S = V.curves(volume_covers(B), 3, 4095).sum(axis=0)
    return V.stream_bits(int(S[0]) // 2 if gated else (int(S[1]) + int(S[2])) // 2, B)


# ------------------------------------------------------------------ blind
@functools.lru_cache(maxsize=None)
def _blind_base(k: int, bright: bool) -> np.ndarray:
    img = CS.planted(H, W, k) if k else CS.smooth(H, W)
    if bright:   # pee_blind_auto_cases.bright's block: candidates at the end of the range, their class depends on T
        img[4:12, 40:56] = np.clip(4095 - 2 + np.random.default_rng(9).integers(-1, 3, (8, 16)), 0, 4095).astype(img.dtype)
    return _frozen(img)


@functools.lru_cache(maxsize=None)
def blind_cover(b: int) -> np.ndarray:
    img = _blind_base(3 + (b // 5) % 2 if b % 5 == 4 else 0, b % 11 == 10).copy()
    rng = np.random.default_rng(90 + b)   # the nudge of tests/test_pee_blind_auto.py's _slice
    ys, xs = rng.integers(H // 2, H - 8, 12), rng.integers(0, W, 12)
    img[ys, xs] = np.clip(img[ys, xs].astype(np.int64) + rng.integers(-1, 2, 12), 0, 4095).astype(img.dtype)
    return _frozen(img)


@functools.lru_cache(maxsize=None)
def blind(b: int):
    """(cover, bits, stego, info, capacity) at BLIND_T, checksum=True"""
    c = blind_cover(b)
    cap = BS.capacity(c, BLIND_T, 4095, BLIND_ME)
    bits = payload(length(b, cap), 7000 + b)
    st, info, _p = BS.embed(c, bits, BLIND_T, 4095, True, BLIND_ME)
    return c, bits, _frozen(st), tuple(int(v) for v in info), cap


@functools.lru_cache(maxsize=None)
def blind_auto(b: int):
    """(cover, bits, stego, info, T, curve) at tmax = TMAX, checksum=True"""
    c = blind_cover(b)
    curve = BAS.capacity_curve(c, TMAX, 4095, BLIND_ME)
    bits = payload(auto_length(b, curve), 8000 + b)
    st, info, T, _p = BAS.embed(c, bits, TMAX, 4095, True, BLIND_ME)
    return c, bits, _frozen(st), tuple(int(v) for v in info), T, curve


@functools.lru_cache(maxsize=None)
def blind_keyed(b: int, B: int, auto_t: bool, nonce: bytes = NONCE):
    """(cover, bits, stego, info, T): fixed BLIND_T (T = BLIND_T whatever the status), or tmax = TMAX"""
    c = blind_cover(b)
    g = index0(B) + b
    if auto_t:
        curve = [BKS.capacity(c, T, 4095, BLIND_ME) for T in range(1, TMAX + 1)]
        bits = payload(auto_length(b, curve), 9000 + b)
        st, info, T, _tag = BKS.embed_auto(c, bits, TMAX, KEY, nonce, g, 4095, BLIND_ME)
    else:
        bits = payload(length(b, BKS.capacity(c, BLIND_T, 4095, BLIND_ME)), 9500 + b)
        st, info, _p, _tag = BKS.embed(c, bits, BLIND_T, KEY, nonce, g, 4095, BLIND_ME)
        T = BLIND_T
    return c, bits, _frozen(st), tuple(int(v) for v in info), T


# ------------------------------------------------------------------ the persistent-grid case
@functools.lru_cache(maxsize=None)
def grid_pair(q: int):
    """(cover, bits) q of the nine the 258 x 512 gated in-place batch cycles over (T_FIXED, G = 24)"""
    c = _frozen(synth.ct12(*GRID_SHAPE, SEED + 500 + q))
    return c, payload(length(q, G.embed(c, [], T_FIXED, 24, 4095)[1]["capacity"]), 9900 + q)


# ------------------------------------------------------------------ what the host test looks at
def _rows(make, B, *, stego, status, end, n, extra=None):
    out = []
    for b in range(B):
        r = make(b)
        out.append({"cover": r[0], "n": len(r[n]), "stego": r[stego], "status": status(r), "end": end(r),
                    "info": extra(r) if extra else ()})
    return out


def _side(i):
    return dict(stego=i - 1, status=lambda r: r[i]["status"], end=lambda r: r[i]["end"], n=1)


def _end2(r, i):
    """scheme 2: the furthest `end` of the four passes (each on its own lattice of about NC candidates)"""
    return max(ps["end"] for ps in r[i]["passes"])


# family -> (the batches it runs at, rows(B)); every row: cover, n (payload bits), stego, status
# (0: embedded; else overflowed / refused), end, info (what tells refused slices apart)
FAMILIES = {
    "fixed-uint16": (("below", "fills", "ragged", "two_rounds"), lambda B: _rows(lambda b: fixed("uint16", b), B, **_side(3))),
    "fixed-uint8": (("below", "fills", "ragged", "two_rounds"), lambda B: _rows(lambda b: fixed("uint8", b), B, **_side(3))),
    "auto-uint16": (("fills", "ragged"), lambda B: _rows(lambda b: auto("uint16", b), B, **_side(4))),
    "auto-uint8": (("fills", "ragged"), lambda B: _rows(lambda b: auto("uint8", b), B, **_side(4))),
    "scheme2": (("fills", "ragged"), lambda B: _rows(lambda b: scheme2("uint16", b), B, stego=2, n=1,
                                                     status=lambda r: r[3]["status"], end=lambda r: _end2(r, 3))),
    "scheme2-auto": (("fills", "ragged"), lambda B: _rows(lambda b: scheme2_auto("uint16", b), B, stego=3, n=1,
                                                          status=lambda r: r[4]["status"], end=lambda r: _end2(r, 4),
                                                          extra=lambda r: (r[2],))),
    "checksum": (("ragged",), lambda B: _rows(lambda b: fixed("uint16", b), B, **_side(3))),
    "keyed": (("fills", "ragged"), lambda B: _rows(lambda b: keyed(b, B), B, **_side(5))),
    "gate-uint16": (("fills", "ragged"), lambda B: _rows(lambda b: gate("uint16", b), B, **_side(5))),
    "gate-uint8": (("fills", "ragged"), lambda B: _rows(lambda b: gate("uint8", b), B, **_side(5))),
    "gate-auto": (("fills", "ragged"), lambda B: _rows(lambda b: gate_auto(b), B, **_side(5))),
    "roi": (("fills", "ragged"), lambda B: _rows(lambda b: roi(b), B, **_side(6))),
    "blind": (("fills", "ragged"), lambda B: _rows(lambda b: blind(b), B, stego=2, n=1, status=lambda r: r[3][0],
                                                   end=lambda r: r[3][4], extra=lambda r: r[3])),
    "blind-auto": (("fills", "ragged"), lambda B: _rows(lambda b: blind_auto(b), B, stego=2, n=1, status=lambda r: r[3][0],
                                                        end=lambda r: r[3][4], extra=lambda r: r[3] + (r[4],))),
    "blind-keyed": (("ragged",), lambda B: _rows(lambda b: blind_keyed(b, B, False), B, stego=2, n=1,
                                                 status=lambda r: r[3][0], end=lambda r: r[3][4], extra=lambda r: r[3])),
    "blind-keyed-auto": (("ragged",), lambda B: _rows(lambda b: blind_keyed(b, B, True, NONCE_2), B, stego=2, n=1,
                                                      status=lambda r: r[3][0], end=lambda r: r[3][4],
                                                      extra=lambda r: r[3] + (r[4],))),
    "quality": (("ragged",), lambda B: _rows(lambda b: fixed("uint16", b), B, **_side(3))),
}
BLIND_FAMILIES = ("blind", "blind-auto", "blind-keyed", "blind-keyed-auto")


def digest(row) -> bytes:
    """What must differ between any two slices of a batch: the stego, and for a slice whose stego is
    its cover (nothing embedded) the cover with its length and info"""
    same = np.array_equal(row["stego"], row["cover"])
    return row["stego"].tobytes() + (repr((row["n"], row["status"], row["info"])).encode() if same else b"")


def volume_plan(B: int, policy: str):
    """(covers, bits, the spec's plan, stegos, sides) of the ungated volume"""
    cov, bits = volume_covers(B), volume_bits(B)
    p = V.plan(V.curves(cov, GATE_TMAX, 4095), len(bits), policy)
    stegos, sides = V.oracle_embed(cov, bits, p, 4095)
    return cov, bits, p, stegos, sides


def gvol_plan(B: int, policy: str):
    """the same for gate="auto" (pee_gvol_spec)"""
    cov, bits = volume_covers(B), volume_bits(B, True)
    p = GV.plan(GV.tables_of(cov, GATE_TMAX, 4095, None), len(bits), policy, None)
    stegos, sides = GV.oracle_embed(cov, bits, p, 4095)
    return cov, bits, p, stegos, sides

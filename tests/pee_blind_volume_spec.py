"""Specification of blind volume payloads (include/codec_tcc_blind_vol.h): one bitstream
planned across a stack of blind MED-PEE stegos, each of which names its place in the stream.  TEST
INFRASTRUCTURE ONLY: the kernels of codec_tcc_amd/csrc/codec_bvol.hip are checked bit-exact against
plan() / embed() / order() / decode(), and those against the scalar restatement at the end of this
file (plain Python loops and ints).  Pure numpy; it composes tests/pee_blind_auto_spec.py (the
per-slice embed with T chosen) with the rule of tests/pee_volume_spec.py (shares and offsets).

  frame     six 32-bit words, LSB first, the first 192 user bits of a carrier: 0 volume_id; 1 the slice's
            index b; 2 B (bits 0-15) | frame flags (bit 16: word 5 holds the stream's CRC); 3 off_b;
            4 N; 5 zlib CRC-32 of the stream's ceil(N / 8) bytes (LSB first, pad bits zero), or 0
  header    the blind header with flag bit 2 (value 4) set in word 1; n_user = 192 + n_b
  transform c[b][T-1] = curve[b][T-1] - 192 where the blind capacity curve is >= 192, else 0
  plan      pee_volume_spec.plan(c, N, policy) for 1 <= N <= 2^31 - 1, except that S(tmax) < N REFUSES
            the volume (status 1): n = off = 0 everywhere, every slice copied through, no header
  skipped   n_b = 0: the slice is its cover, no header; per-slice info (3, 0, 0, 0, -1, 0), T 0
  carrier   pee_blind_auto_spec.embed(cover, frame || share, tmax, ...) with flag bit 2 set.  A T exists:
            the status-0 lengths of a blind plan at one T are downward closed (the host test shows it
            by brute force on its cases), and 192 + n_b <= curve[b][T*-1]
  order     status 0 ok; 1 no carrier; 2 carriers that differ from the first (stack order) in words 0,
            2, 4 or 5, or a first frame with B = 0 or N outside 1..2^31-1; 3 an index >= B, a share past
            N, two carriers with one index, or shares that overlap when taken in index order; 4 a gap.
            missing: the maximal ranges [lo, hi) of [0, N) no carrier covers (status 0 and 4)
  decode    any slice order; a slice without the magic is no carrier and is returned as it is
"""
from __future__ import annotations

import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

try:   # with tests/ on the path (the suite, the golden generator) or as tests.pee_blind_volume_spec
    import pee_blind_auto_spec as AS
    import pee_blind_spec as BS
    import pee_volume_spec as VS
except ImportError:   # pragma: no cover
    from tests import pee_blind_auto_spec as AS, pee_blind_spec as BS, pee_volume_spec as VS

FLAG_VOLUME = 4
FRAME_WORDS = 6
FRAME_BITS = 32 * FRAME_WORDS
FRAME_CRC = 1 << 16
MAX_B = 65535
NMAX = 2 ** 31 - 1
SKIPPED = 3
SKIPPED_INFO = (SKIPPED, 0, 0, 0, -1, 0)
OK, NO_CARRIER, MIXED, OVERLAP, GAP = 0, 1, 2, 3, 4


def transform(curve) -> np.ndarray:
    curve = np.asarray(curve, dtype=np.int64)
    return np.where(curve >= FRAME_BITS, curve - FRAME_BITS, 0)


def stream_crc(bits) -> int:
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    return zlib.crc32(np.packbits(bits, bitorder="little").tobytes()) & 0xFFFFFFFF


def frame(volume_id: int, b: int, B: int, off: int, N: int, crc: Optional[int]) -> List[int]:
    return [int(volume_id) & 0xFFFFFFFF, int(b), int(B) | (FRAME_CRC if crc is not None else 0), int(off), int(N),
            int(crc) if crc is not None else 0]


def curves(covers, tmax: int, maxval=None, max_entries: int = 256) -> np.ndarray:
    return np.array([AS.capacity_curve(c, tmax, maxval, max_entries) for c in covers], dtype=np.int64)


def plan(curve, N: int, policy: str = "even") -> Dict:
    """status, T (= T*), capacity (= S(T*)), capacity_max (= S(tmax)), carriers, n[B], off[B]."""
    N = int(N)
    if not 1 <= N <= NMAX:
        raise ValueError("N must be in 1..2^31 - 1")
    c = transform(curve)
    if c.shape[0] > MAX_B:
        raise ValueError("B must be <= 65535")
    p = VS.plan(c, N, policy)
    B = c.shape[0]
    if p["status"]:
        n, off = np.zeros(B, np.int64), np.zeros(B, np.int64)
    else:
        n, off = p["n"], p["off"][:B]
    return {"status": p["status"], "T": p["T"], "capacity": p["capacity"], "capacity_max": int(c[:, -1].sum()),
            "carriers": int((n > 0).sum()), "N": N, "policy": policy, "n": n, "off": off}


def set_volume_flag(stego: np.ndarray) -> None:
    """Header word 1, bit 10 (flags bit 2): side bit 42, the LSB of pixel H W - 1 - 42."""
    flat = stego.ravel()
    flat[flat.size - 1 - 42] |= 1


def clear_volume_flag(stego: np.ndarray) -> None:
    flat = stego.ravel()
    flat[flat.size - 1 - 42] &= ~np.asarray(1, stego.dtype)


def embed(covers, bits, *, volume_id: int, policy: str = "even", tmax: int = 8, maxval=None, checksum: bool = False,
          max_entries: int = 256) -> Dict:
    """stegos [B,H,W], plan, infos [B] (6-tuples), ts [B], frames [B][6] (zero rows for skipped slices).
    checksum: the covers' CRCs in the headers and the stream's in the frames."""
    covers = np.asarray(covers)
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    B = covers.shape[0]
    p = plan(curves(covers, tmax, maxval, max_entries), bits.size, policy)
    crc = stream_crc(bits) if checksum else None
    stegos, infos, ts, frames = [], [], [], []
    for b in range(B):
        nb, ob = int(p["n"][b]), int(p["off"][b])
        if nb == 0:
            stegos.append(covers[b].copy()); infos.append(SKIPPED_INFO); ts.append(0); frames.append([0] * FRAME_WORDS)
            continue
        f = frame(volume_id, b, B, ob, bits.size, crc)
        user = np.concatenate([BS.words_to_bits(f), bits[ob:ob + nb]])
        st, info, T, _p = AS.embed(covers[b], user, tmax, maxval, checksum, max_entries)
        assert T != 0 and info[0] == 0, (b, nb, info)
        set_volume_flag(st)
        stegos.append(st); infos.append(tuple(int(v) for v in info)); ts.append(T); frames.append(f)
    return {"stego": np.stack(stegos), "plan": p, "info": infos, "ts": ts, "frames": frames}


def missing_ranges(intervals: Sequence[Tuple[int, int]], N: int) -> List[Tuple[int, int]]:
    out, at = [], 0
    for lo, hi in sorted(intervals):
        if lo > at:
            out.append((at, lo))
        at = max(at, hi)
    if at < N:
        out.append((at, N))
    return out


def order(frames, n) -> Dict:
    """frames: the carriers' six words in stack order; n: their share lengths."""
    frames = [[int(v) & 0xFFFFFFFF for v in f] for f in frames]
    n = [int(v) for v in n]
    out = {"status": OK, "carriers": len(frames), "N": 0, "B": 0, "volume_id": 0, "crc": None, "missing": [], "by_index": {}}
    if not frames:
        out["status"] = NO_CARRIER
        return out
    ref = frames[0]
    B, N = ref[2] & 0xFFFF, ref[4]
    if B < 1 or not 1 <= N <= NMAX or any([f[0], f[2], f[4], f[5]] != [ref[0], ref[2], ref[4], ref[5]] for f in frames):
        out["status"] = MIXED
        return out
    out.update(N=N, B=B, volume_id=ref[0], crc=ref[5] if ref[2] & FRAME_CRC else None)
    idx = [f[1] for f in frames]
    if any(i >= B for i in idx) or any(f[3] + nb > N for f, nb in zip(frames, n)) or len(set(idx)) != len(idx):
        out["status"] = OVERLAP
        return out
    by = sorted(zip(idx, [f[3] for f in frames], n, range(len(frames))))
    end = 0
    for _i, off, nb, _k in by:
        if off < end:
            out["status"] = OVERLAP
            return out
        end = max(end, off + nb)
    out["by_index"] = {i: (off, nb, k) for i, off, nb, k in by}
    out["missing"] = missing_ranges([(off, off + nb) for _i, off, nb, _k in by], N)
    if out["missing"]:
        out["status"] = GAP
    return out


def decode(stegos, partial: bool = False, verify: bool = True):
    """(stream bits, covers, order dict).  ValueError for a refused stack (IntegrityError's place is
    the codec's: here a CRC mismatch is a ValueError too)."""
    covers, frames, n, shares = [], [], [], []
    for st in stegos:
        st = np.asarray(st)
        H, W = st.shape
        w = [int(v) for v in BS.read_words(st, 0, 2)] if H * W >= BS.HDR_BITS else [0, 0]
        if w[0] != BS.MAGIC:
            covers.append(st.copy())
            continue
        flags = (w[1] >> 8) & 0xFF
        if not flags & FLAG_VOLUME or flags & ~(FLAG_VOLUME | BS.FLAG_CRC):
            raise ValueError(f"flags = {flags:#x}: no volume slice")
        plain = st.copy()
        clear_volume_flag(plain)
        user, cover, h = BS.decode(plain, verify)
        if h["n_user"] < FRAME_BITS:
            raise ValueError("n_user < 192: no frame")
        covers.append(cover)
        frames.append([int(v) for v in BS.bits_to_words(user[:FRAME_BITS])])
        n.append(user.size - FRAME_BITS)
        shares.append(user[FRAME_BITS:])
    o = order(frames, n)
    if o["status"] not in (OK, GAP) or (o["status"] == GAP and not partial):
        raise ValueError(f"blind volume: status {o['status']}, missing {o['missing']}")
    bits = np.zeros(o["N"], np.uint8)
    for _i, (off, nb, k) in o["by_index"].items():
        bits[off:off + nb] = shares[k]
    if verify and o["status"] == OK and o["crc"] is not None and stream_crc(bits) != o["crc"]:
        raise ValueError("the stream fails the frames' CRC")
    return bits, np.stack(covers), o


# ---------------------------------------------------------------- the tests' stacks
def smooth(h: int, w: int, seed: int, dtype="uint16") -> np.ndarray:
    """pee_blind_cases.smooth with its own seed: the ct12 field + N(0, 1.5), rounded and clipped."""
    y, x = np.mgrid[0:h, 0:w]
    f = (np.sin(x / 97.0 + seed) + np.cos(y / 61.0) + 2.0) / 4.0 * 4095.0 * 0.8
    top = 4095 if np.dtype(dtype) == np.uint16 else 255
    if np.dtype(dtype) == np.uint8:
        f = f / 16.0
    return np.clip(np.rint(f + np.random.default_rng(seed).normal(0.0, 1.5, (h, w))), 0, top).astype(dtype)


def checker(h: int, w: int, dtype="uint16") -> np.ndarray:
    """0 / maximum in a one-pixel checkerboard: no candidate expands, the blind capacity is -1."""
    top = 4095 if np.dtype(dtype) == np.uint16 else 255
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * top).astype(dtype)


def stack(B: int, h: int, w: int, dtype="uint16", checker_at: int = 1, seed: int = 300) -> np.ndarray:
    """B slices: smooth covers of distinct seeds, slice `checker_at` the checkerboard (the non-carrier)."""
    out = [checker(h, w, dtype) if b == checker_at else smooth(h, w, seed + b, dtype) for b in range(B)]
    return np.stack(out)


def stream_bits(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(8000 + seed).integers(0, 2, int(n)).astype(np.uint8)


# ---------------------------------------------------------------- scalar restatement (the new parts)
def transform_scalar(curve: List[List[int]]) -> List[List[int]]:
    return [[(int(v) - 192) if int(v) >= 192 else 0 for v in row] for row in curve]


def frame_bits_scalar(volume_id: int, b: int, B: int, off: int, N: int, crc: Optional[int]) -> List[int]:
    words = [volume_id, b, B + (65536 if crc is not None else 0), off, N, crc if crc is not None else 0]
    out = []
    for w in words:
        for j in range(32):
            out.append((int(w) >> j) & 1)
    return out


def plan_scalar(curve: List[List[int]], N: int, policy: str = "even") -> Dict:
    c = transform_scalar(curve)
    B, tmax = len(c), len(c[0])
    S = [sum(c[b][k] for b in range(B)) for k in range(tmax)]
    T = next((k + 1 for k in range(tmax) if S[k] >= N), 0)
    if T == 0:
        return {"status": 1, "T": tmax, "capacity": S[-1], "capacity_max": S[-1], "carriers": 0, "n": [0] * B, "off": [0] * B}
    PB, Pb, n, off = S[T - 1], 0, [], []
    for b in range(B):
        cb = c[b][T - 1]
        if policy == "even":
            lo, hi = N * Pb // PB, N * (Pb + cb) // PB
        else:
            lo = min(N, Pb)
            hi = lo + min(cb, N - lo)
        off.append(lo); n.append(hi - lo)
        Pb += cb
    return {"status": 0, "T": T, "capacity": PB, "capacity_max": S[-1], "carriers": sum(1 for v in n if v > 0), "n": n,
            "off": off}


def order_scalar(frames: List[List[int]], n: List[int]) -> Tuple[int, List[Tuple[int, int]]]:
    """(status, missing) by marking every stream bit."""
    if not frames:
        return NO_CARRIER, []
    ref = frames[0]
    B, N = ref[2] % 65536, ref[4]
    if B == 0 or N < 1 or N > NMAX:
        return MIXED, []
    for f in frames:
        for k in (0, 2, 4, 5):
            if f[k] != ref[k]:
                return MIXED, []
    seen = {}
    for k, f in enumerate(frames):
        if f[1] >= B or f[3] + n[k] > N or f[1] in seen:
            return OVERLAP, []
        seen[f[1]] = k
    marks = [0] * N
    last_end = 0
    for i in sorted(seen):
        k = seen[i]
        if frames[k][3] < last_end:
            return OVERLAP, []
        for q in range(frames[k][3], frames[k][3] + n[k]):
            marks[q] += 1
        last_end = max(last_end, frames[k][3] + n[k])
    missing, q = [], 0
    while q < N:
        if marks[q] == 0:
            lo = q
            while q < N and marks[q] == 0:
                q += 1
            missing.append((lo, q))
        else:
            q += 1
    return (GAP if missing else OK), missing

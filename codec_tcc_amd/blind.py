"""Blind MED-PEE (include/codec_tcc_blind.h): the stego alone carries its location map
and record, so that it decodes with nothing beside it.

    stego, info = codec.embed_blind(covers, payloads, checksum=True)
    bits, cover = codec.decode_blind(stego)              # T and maxval come from each header

Scheme 1, fixed T, out of place, per slice.  A slice carries n_side = 192 + 32 E side bits in the
LSBs of its last pixels (side bit i = bit 0 of the pixel with flat index H W - 1 - i): six header
words, then the E location-map entries.  Those pixels lie in a region the ROI embed
(include/codec_tcc_roi.h) neither modifies nor reads as context, and the LSBs they displace lead
the PEE payload.  The plan -- which rows the payload needs, hence E and the region -- is computed
on the device from the cover alone (tests/pee_blind_spec.py is the specification).

Capacity control (include/codec_tcc_blind_auto.h): embed_auto picks, per slice and on
the device, the smallest T in 1..tmax whose plan succeeds; the format and the decode are the same.

    stego, info, ts = codec.embed_blind_auto(covers, payloads, tmax=8)

Keyed (include/codec_tcc_blind_keyed.h): the user bits of a slice with flag bit 1 are a
224-bit frame (nonce12, Poly1305 tag) and the ChaCha20 ciphertext, so a 32-byte key is all a reader
needs besides the pixels; tests/pee_blind_keyed_spec.py is the specification.

    stego, info, ts = codec.embed_blind_keyed(covers, payloads, key=key)
    bits, cover = codec.decode_blind_keyed(stego, key)

Gated (include/codec_tcc_blind_gate.h): embed_gated picks, per slice and on the device,
the pair (T, gate) -- the smallest T for which some gate of the ladder _lib.GATES has a plan, and at
that T the smallest such gate; only candidates whose MED context is that flat are modified.  The gate
rides in the header (flag bit 3, its ladder index in flag bits 4-7) and decode reads gated and
ungated slices alike; tests/pee_blind_gate_spec.py is the specification.

    stego, info, ts, gs = codec.embed_blind_gated(covers, payloads, tmax=8)

parse_header, check_args and the geometry helpers are pure host code: no GPU, no library load.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import numpy as np

from . import _lib

MAGIC = _lib.BLIND_MAGIC
HDR_WORDS = _lib.BLIND_HDR_WORDS
HDR_BITS = 32 * HDR_WORDS
NO_ENTRY = 0xFFFFFFFF
FLAG_CRC = _lib.BLIND_FLAG_CRC
FLAG_KEYED = _lib.BLIND_FLAG_KEYED
KEYED_FRAME_BITS = _lib.BLIND_FRAME_BITS
FLAG_VOLUME = _lib.BLIND_FLAG_VOLUME
VOLUME_FRAME_BITS = _lib.BVOL_FRAME_BITS
FLAG_GATED = _lib.BLIND_FLAG_GATED
FLAG_GATE_SHIFT = _lib.BLIND_FLAG_GATE_SHIFT
FLAG_GATE_MASK = 15 << FLAG_GATE_SHIFT
GATES = _lib.GATES
GATED_TMAX_DEFAULT = 4
MAX_ENTRIES = _lib.BLIND_MAX_ENTRIES
MAX_DIM = _lib.ROI_MAX_DIM
TMAX = _lib.BLIND_TMAX
INFO_FIELDS = ("status", "n_user", "E", "n_side", "end", "region_row")
STATUS_TEXT = {1: "the payload and its side bits exceed the slice's capacity",
               2: "more location-map entries than max_entries"}


def side_bits(E: int) -> int:
    return HDR_BITS + 32 * int(E)


def region(H: int, W: int, n_side: int) -> Tuple[int, Tuple[int, int, int, int]]:
    """(r, rectangle): the candidate rows and the pixel rectangle reserved for n_side side bits."""
    r = -(-int(n_side) // (2 * int(W)))
    return r, (2 * (int(H) // 2 - r), 0, int(H), int(W))


def row_words(n_user: int, max_entries: int) -> int:
    """uint64 words of the PEE payload row: CODEC_PEE_BLIND_ROW_WORDS."""
    return (int(n_user) + HDR_BITS + 32 * int(max_entries) + 63) // 64


def check_args(*, scheme: int, T, gate, H: int, W: int, maxval: int, max_entries: int = 256, roi=None, key=None,
               in_place: bool = False) -> None:
    """The argument rules of the blind calls, as ValueError before anything is queued, in this
    order: scheme, T, gate, roi / key, the shape, maxval, max_entries, in place."""
    if int(scheme) != 1:
        raise ValueError("blind MED-PEE is scheme 1's: scheme 2's later passes modify the pixels that hold the side bits "
                         "(DESIGN §3k)")
    if isinstance(T, str):
        raise ValueError("blind MED-PEE takes a fixed T: the plan needs one row table per T (DESIGN §3k)")
    if not 1 <= int(T) <= 64:
        raise ValueError(f"blind MED-PEE takes T in 1..64, got {T}")
    if gate is not None:
        raise ValueError("blind MED-PEE takes no smoothness gate: the plan counts every candidate (DESIGN §3k)")
    if roi is not None:
        raise ValueError("blind MED-PEE takes no roi=: the reserved region is the slice's one rectangle (DESIGN §3k)")
    if key is not None:
        raise ValueError("blind MED-PEE takes no key=: the header has no room for the tag (DESIGN §3k)")
    if int(H) > MAX_DIM or int(W) > MAX_DIM:
        raise ValueError(f"blind MED-PEE takes H, W <= {MAX_DIM} (the ROI record words), got {int(H)} x {int(W)}")
    if int(H) * int(W) < HDR_BITS:
        raise ValueError(f"a {int(H)} x {int(W)} slice cannot hold the {HDR_BITS} header bits")
    if not 1 <= int(maxval) <= 65535:
        raise ValueError(f"the header holds maxval in 1..65535, got {maxval}")
    if isinstance(max_entries, bool) or int(max_entries) != max_entries or not 0 <= int(max_entries) <= MAX_ENTRIES:
        raise ValueError(f"max_entries must be an integer in 0..{MAX_ENTRIES}, got {max_entries!r}")
    if in_place:
        raise ValueError("blind MED-PEE embeds out of place only: pass a stego buffer other than the covers")


def check_args_auto(*, scheme: int, tmax, gate, H: int, W: int, maxval: int, max_entries: int = 256, roi=None, key=None,
                    in_place: bool = False) -> None:
    """check_args for the calls that choose T: the same rules in the same order, with tmax in
    1..16 in T's place."""
    if int(scheme) == 1 and (isinstance(tmax, (bool, str)) or int(tmax) != tmax or not 1 <= int(tmax) <= TMAX):
        raise ValueError(f"blind MED-PEE chooses T in 1..tmax with tmax an integer in 1..{TMAX}, got {tmax!r}")
    check_args(scheme=scheme, T=1, gate=gate, H=H, W=W, maxval=maxval, max_entries=max_entries, roi=roi, key=key,
               in_place=in_place)


def _flags_error(flags: int, n_user: int, keyed: bool, volume: bool = False):
    """The reason (or None) the flags of a header are refused: unkeyed, bit 0 and the gate's fields
    are defined (bit 3, and bits 4-7 beside it: DESIGN §3o); keyed, they are exactly FLAG_KEYED and
    n_user holds the frame; volume, they are FLAG_VOLUME with or without bit 0 and
    n_user holds the 192-bit volume frame."""
    if volume:
        if keyed or (flags & ~FLAG_CRC) != FLAG_VOLUME:
            return f"flags = {flags:#x} (a volume slice has bit 2, and bit 0 at most beside it)"
        if n_user < VOLUME_FRAME_BITS:
            return f"n_user = {n_user} (a volume slice holds the {VOLUME_FRAME_BITS} frame bits)"
        return None
    if not keyed:
        if flags & ~(FLAG_CRC | FLAG_GATED | FLAG_GATE_MASK):
            return f"flags = {flags:#x} (bit 0 alone is defined)" if not flags & (FLAG_GATED | FLAG_GATE_MASK) else \
                f"flags = {flags:#x} (bits 0 and 3 alone are defined, and bits 4-7 beside bit 3)"
        if flags & FLAG_GATE_MASK and not flags & FLAG_GATED:
            return f"flags = {flags:#x} (bits 4-7 hold a gate only beside bit 3)"
        return None
    if flags != FLAG_KEYED:
        return (f"flags = {flags:#x} (a keyed slice has exactly {FLAG_KEYED:#x}" +
                ("; an unkeyed stego is decode_blind's)" if not flags & ~FLAG_CRC else ")"))
    if n_user < KEYED_FRAME_BITS:
        return f"n_user = {n_user} (a keyed slice holds the {KEYED_FRAME_BITS} frame bits)"
    return None


def parse_header(words, H: int, W: int, vmax: int, *, keyed: bool = False, volume: bool = False) -> Dict:
    """One slice's six header words -> {T, flags, maxval, n_user, E, end, crc, n_side, rect, L}, and
    "G", the gate, for a gated slice (an ungated slice's dict is what it was);
    ValueError naming the field for anything that is no header of an H x W slice.  keyed=True: the
    header of a keyed slice (flags exactly FLAG_KEYED, n_user >= 224), which the default refuses;
    volume=True: that of a volume slice (flag bit 2, n_user >= 192), which the default refuses too."""
    w = [int(v) & 0xFFFFFFFF for v in list(words)[:HDR_WORDS]]
    H, W = int(H), int(W)
    hc, wc = H // 2, W // 2
    nc = hc * wc
    if w[0] != MAGIC:
        raise ValueError(f"magic = {w[0]:#010x} (a blind MED-PEE header starts with {MAGIC:#010x})")
    T, flags, maxval = w[1] & 0xFF, (w[1] >> 8) & 0xFF, w[1] >> 16
    if not 1 <= T <= 64:
        raise ValueError(f"T = {T} (1..64)")
    why = _flags_error(flags, w[2], keyed, volume)
    if why:
        raise ValueError(why)
    if not 1 <= maxval <= vmax:
        raise ValueError(f"maxval = {maxval} (1..{vmax})")
    n_user, E = w[2], w[3]
    end = -1 if w[4] == NO_ENTRY else w[4]
    if end >= nc:
        raise ValueError(f"end = {end} (the slice has {nc} candidates)")
    n_side = side_bits(E)
    if E > nc or n_side > H * W:
        raise ValueError(f"E = {E} (the slice cannot hold {n_side} side bits)")
    r, rect = region(H, W, n_side)
    if r > hc:
        raise ValueError(f"n_side = {n_side} (more than the slice's {hc} candidate rows hold)")
    if end >= (hc - r) * wc:
        raise ValueError(f"end = {end} (inside the reserved region, which starts at candidate row {hc - r})")
    L = n_side + n_user
    if L > end + 1:
        raise ValueError(f"n_user = {n_user} ({L} bits cannot lie in candidates 0..{end})")
    out = {"T": T, "flags": flags, "maxval": maxval, "n_user": n_user, "E": E, "end": end, "crc": w[5],
           "n_side": n_side, "rect": rect, "L": L}
    if flags & FLAG_GATED:
        out["G"] = GATES[(flags & FLAG_GATE_MASK) >> FLAG_GATE_SHIFT]
    return out


def parse_headers(hdr: np.ndarray, H: int, W: int, nbytes: int, *, keyed: bool = False,
                  volume: bool = False) -> Dict[str, np.ndarray]:
    """Every slice's header (hdr: uint32 [B, >= 6] as codec_pee_blind_headers gathers them) as int64
    arrays [B] under parse_header's names ("rect": [B, 4]; without keywords also "G": the gate of a
    gated slice, _lib.GATE_MAX of any other): parse_header's rules applied to all slices at once.  ValueError naming the slices that carry no header, each with parse_header's
    reason.  keyed, volume: parse_header's."""
    H, W = int(H), int(W)
    hc, wc = H // 2, W // 2
    nc = hc * wc
    vmax = 65535 if int(nbytes) == 2 else 255
    w = np.asarray(hdr)[:, :HDR_WORDS].astype(np.int64) & 0xFFFFFFFF
    T, flags, maxval = w[:, 1] & 0xFF, (w[:, 1] >> 8) & 0xFF, w[:, 1] >> 16
    n_user, E = w[:, 2], w[:, 3]
    end = np.where(w[:, 4] == NO_ENTRY, -1, w[:, 4])
    n_side = HDR_BITS + 32 * E
    r = -(-n_side // (2 * W))
    L = n_side + n_user
    if volume:
        flags_ok = ((flags & ~FLAG_CRC) == FLAG_VOLUME) & (n_user >= VOLUME_FRAME_BITS) & (not keyed)
    else:
        flags_ok = ((flags == FLAG_KEYED) & (n_user >= KEYED_FRAME_BITS)) if keyed else \
            (((flags & ~(FLAG_CRC | FLAG_GATED | FLAG_GATE_MASK)) == 0) & (((flags & FLAG_GATE_MASK) == 0) | ((flags & FLAG_GATED) != 0)))
    ok = ((w[:, 0] == MAGIC) & (T >= 1) & (T <= 64) & flags_ok & (maxval >= 1) & (maxval <= vmax)
          & (end < nc) & (E <= nc) & (n_side <= H * W) & (r <= hc) & (end < (hc - r) * wc) & (L <= end + 1))
    if not ok.all():
        bad = []
        for b in np.flatnonzero(~ok):
            try:
                parse_header(w[b], H, W, vmax, keyed=keyed, volume=volume)
                bad.append((int(b), "inconsistent header"))   # (the two statements of the rules disagree)
            except ValueError as e:
                bad.append((int(b), str(e)))
        raise ValueError(f"no valid {'keyed ' if keyed else 'volume ' if volume else ''}blind MED-PEE header in slices {[b for b, _ in bad]}: "
                         + "; ".join(f"slice {b}: {why}" for b, why in bad[:4]))
    rect = np.stack([2 * (hc - r), np.zeros_like(r), np.full_like(r, H), np.full_like(r, W)], axis=1)
    out = {"T": T, "flags": flags, "maxval": maxval, "n_user": n_user, "E": E, "end": end, "crc": w[:, 5],
           "n_side": n_side, "rect": rect, "L": L}
    if not keyed and not volume:   # those refuse a gated slice: their arrays are what they were
        out["G"] = np.where((flags & FLAG_GATED) != 0, np.asarray(GATES, np.int64)[(flags & FLAG_GATE_MASK) >> FLAG_GATE_SHIFT],
                            _lib.GATE_MAX)
    return out


def records_bytes(heads: Dict[str, np.ndarray], H: int, W: int) -> bytes:
    """The codec_pee_meta records of checked headers, as pee_checks.make_record(..., status=0, roi=rect)
    writes them (B records of 16 int32 words), built for all slices at once; reserved[1] is each
    slice's gate + 1 (65536 for an ungated one, and for headers parsed without a "G")."""
    B = heads["T"].shape[0]
    nc = (int(H) // 2) * (int(W) // 2)
    m = np.zeros((B, _lib.PEE_META_BYTES // 4), dtype=np.int64)
    end, rect = heads["end"], heads["rect"]
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = heads["T"], heads["maxval"], heads["L"], end
    m[:, 4], m[:, 5] = nc, (nc + 1023) // 1024
    m[:, 6] = np.where(end >= 0, end // 1024, -1)
    m[:, 8], m[:, 10], m[:, 11] = heads["L"], int(H), int(W)
    m[:, 13] = (rect[:, 0] << 16) | rect[:, 1]
    m[:, 14] = (heads["G"] if "G" in heads else _lib.GATE_MAX) + 1
    m[:, 15] = (rect[:, 2] << 16) | rect[:, 3]
    return (m & 0xFFFFFFFF).astype("<u4").tobytes()


def raise_status(status, what: str = "embed_blind") -> None:
    """ValueError naming the slices an embed refused (info's status column, on the host)."""
    bad: Dict[int, List[int]] = {}
    for b, s in enumerate(status):
        if int(s) != 0:
            bad.setdefault(int(s), []).append(b)
    if bad:
        raise ValueError(f"{what}: " + "; ".join(f"{STATUS_TEXT.get(s, 'status %d' % s)} in slices {v}"
                                                 for s, v in sorted(bad.items())))


# ---------------------------------------------------------------- the device side (PeeCodec's methods call these)
def _workspace(codec, pw: int, max_entries: int, tmax: int = 0):
    """The blind workspace for rows of pw words: a codec_pee workspace with the plan's arrays, a
    map and the rows behind it, zeroed once (codec_pee_reset) and kept (the last few).  tmax > 0:
    the workspace of the calls that choose T, with a row table for every T in 1..tmax."""
    from collections import OrderedDict
    from .codec import _stream, _torch
    cache = codec.__dict__.setdefault("_ws_blind", OrderedDict())
    key = (int(pw), int(max_entries), int(tmax))
    if key not in cache:
        P = _params_auto(codec, pw) if tmax else codec._params(pw)
        if tmax:
            fn = "codec_pee_blind_auto_workspace_bytes"
            n = int(_lib.load().codec_pee_blind_auto_workspace_bytes(C.byref(P), int(tmax), int(max_entries)))
        else:
            fn = "codec_pee_blind_workspace_bytes"
            n = int(_lib.load().codec_pee_blind_workspace_bytes(C.byref(P), int(max_entries)))
        if n == 0:
            _lib.check(-1, fn)
        ws = _torch().empty(n, dtype=_torch().uint8, device=codec.device)
        _lib.check(_lib.load().codec_pee_reset(C.byref(P), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_reset")
        cache[key] = ws
        while len(cache) > 4:
            cache.popitem(last=False)
    cache.move_to_end(key)
    return cache[key]


def _params_auto(codec, pw: int):
    """The codec's parameters with T = 1: the calls that choose T only range-check it."""
    P = codec._params(pw)
    P.T = 1
    return P


def _guarded(codec, ws, pw: int, fn):
    """Run one call on a blind workspace; on any exception re-zero that workspace, then re-raise."""
    from .codec import _stream
    try:
        return fn()
    except BaseException:
        try:
            _lib.load().codec_pee_reset(C.byref(codec._params(pw)), ws.data_ptr(), ws.numel(), _stream())
        except Exception:   # the original error is the one to report
            pass
        raise


def _codec_args(codec, max_entries: int = 256, in_place: bool = False):
    check_args(scheme=codec.scheme, T="auto" if codec.auto else codec.T, gate=codec.gate, H=codec.H, W=codec.W,
               maxval=codec.maxval, max_entries=max_entries, in_place=in_place)


def embed(codec, covers, payloads, *, stego=None, packed=None, checksum=False, max_entries: int = 256,
          check: bool = True):
    from . import checksum as _ck
    from .codec import _stream, _torch
    from .pee_checks import check_buffers
    torch = _torch()
    if checksum not in (False, True):
        raise ValueError("embed_blind takes checksum=True or False (the header holds the cover's CRC-32 alone)")
    _codec_args(codec, max_entries)
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  covers=covers, stego=stego, packed=packed)
    _codec_args(codec, max_entries, in_place=stego is not None and stego.data_ptr() == covers.data_ptr())
    words, lengths, lens_t = packed if packed is not None else codec.pack_payloads(payloads)
    n_max = max([int(n) for n in lengths] + [0])
    if n_max > 64 * int(words.shape[1]):
        raise ValueError(f"a payload of {n_max} bits does not fit the packed rows' {64 * int(words.shape[1])}")
    pw = row_words(n_max, max_entries)
    crc = _ck.crc32_slices(covers) if checksum else None   # queued first, as embed(checksum=True) does
    if stego is None:
        stego = torch.empty_like(covers)
    ws = _workspace(codec, pw, max_entries)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    lm = torch.empty((codec.B, codec.lm_words), dtype=torch.int64, device=codec.device)
    meta = torch.empty((codec.B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=codec.device)
    P = codec._params(pw)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_embed(
        C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), int(words.shape[1]), lens_t.data_ptr(),
        None if crc is None else crc.data_ptr(), int(max_entries), info.data_ptr(), meta.data_ptr(), lm.data_ptr(),
        ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_embed"))
    out = info[:, :len(INFO_FIELDS)]
    if check:
        raise_status(out[:, 0].cpu().tolist())   # one read-back
    return stego, out


def capacity(codec, covers, max_entries: int = 256):
    from .codec import _stream, _torch
    torch = _torch()
    _codec_args(codec, max_entries)
    codec._check_buffers(covers=covers)
    pw = row_words(0, max_entries)
    ws = _workspace(codec, pw, max_entries)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_plan(
        C.byref(codec._params(pw)), covers.data_ptr(), None, int(max_entries), info.data_ptr(), ws.data_ptr(), ws.numel(),
        _stream()), "codec_pee_blind_plan"))
    return info[:, _lib.BLIND_INFO_WORDS - 1].contiguous()


def _headers(codec, stego, cover, *, keyed: bool = False):
    """(hdr, heads): the buffers judged, every slice's header gathered on the device and read back
    once (hdr: the device tensor, heads: parse_headers' arrays)."""
    from .codec import _stream, _torch
    from .pee_checks import check_buffers
    torch = _torch()
    if codec.scheme != 1:
        raise ValueError("blind MED-PEE is scheme 1's")
    if codec.H > MAX_DIM or codec.W > MAX_DIM or codec.H * codec.W < HDR_BITS:
        raise ValueError(f"a {codec.H} x {codec.W} slice carries no blind MED-PEE header")
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  stego=stego, cover=cover)
    if cover is not None and cover.data_ptr() == stego.data_ptr():
        raise ValueError("blind MED-PEE decodes out of place only: pass a cover buffer other than the stego")
    hdr = torch.empty((codec.B, 8), dtype=torch.int32, device=codec.device)
    _lib.check(_lib.load().codec_pee_blind_headers(C.byref(codec._params(1)), stego.data_ptr(), hdr.data_ptr(), _stream()),
               "codec_pee_blind_headers")
    # the one read-back before the extract
    return hdr, parse_headers(hdr.cpu().numpy().view(np.uint32), codec.H, codec.W, codec.bytes, keyed=keyed)


def _extract(codec, stego, hdr, heads, cover):
    """(user rows [B, uw] on the device, cover, ws, pw): the records rebuilt from the checked headers
    and judged, then codec_pee_blind_extract queued."""
    from .codec import _stream, _torch
    from .pee_checks import check_records
    torch = _torch()
    pw = max(HDR_BITS // 64, int((heads["L"].max() + 63) // 64))
    uw = max(1, int((heads["n_user"].max() + 63) // 64))
    raw = records_bytes(heads, codec.H, codec.W)
    check_records([_lib.PeeMeta.from_buffer_copy(raw, b * _lib.PEE_META_BYTES) for b in range(codec.B)], codec.H, codec.W,
                  scheme=1, payload_words=pw, lm_words=codec.lm_words, bytes=codec.bytes)
    meta = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy().reshape(codec.B, _lib.PEE_META_BYTES)).to(codec.device)
    if cover is None:
        cover = torch.empty_like(stego)
    words = torch.empty((codec.B, uw), dtype=torch.int64, device=codec.device)
    ws = _workspace(codec, pw, 0)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_extract(
        C.byref(codec._params(pw)), stego.data_ptr(), hdr.data_ptr(), meta.data_ptr(), cover.data_ptr(), words.data_ptr(),
        uw, ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_extract"))
    return words, cover, ws, pw


def _lookback_flag(codec, ws, pw):
    """The flat look-back route's flag word in the workspace (small batches take that route out of
    place too) as an int32 [1] device view, or None when the shape has none."""
    from .codec import _torch
    off = int(_lib.load().codec_pee_extract_flag_offset(C.byref(codec._params(pw))))
    return ws[off:off + 4].view(_torch().int32) if off else None


def _raise_lookback(codec, ws, pw):
    from . import pee_verify as _pv
    from .codec import _stream
    _lib.check(_lib.load().codec_pee_reset(C.byref(codec._params(pw)), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_reset")
    raise RuntimeError(_pv.LOOKBACK_TIMEOUT)


def decode(codec, stego, *, cover=None, verify=True):
    from . import checksum as _ck, framing, pee_verify as _pv
    mode = _ck.verify_mode(verify)
    hdr, heads = _headers(codec, stego, cover)
    has_crc = (heads["flags"] & FLAG_CRC) != 0
    if mode == "require" and not has_crc.all():
        raise _ck.IntegrityError("blind MED-PEE decode: verify='require' and slices "
                                 f"{np.flatnonzero(~has_crc).tolist()} carry no cover checksum")
    words, cover, ws, pw = _extract(codec, stego, hdr, heads, cover)
    flagged = np.flatnonzero(has_crc).tolist()
    got = _ck.crc32_slices(cover) if mode is not None and flagged else None
    host = words.cpu().numpy()
    flag = _lookback_flag(codec, ws, pw)   # as decode() reads it
    if flag is not None and int(flag.item()) != 0:
        _raise_lookback(codec, ws, pw)
    if got is not None:
        bad = set(_pv.cover_mismatches(got, heads["crc"].tolist(), codec.B))
        _ck.raise_mismatch([b for b in flagged if b in bad], [], "blind MED-PEE decode", rows=host)
    n_user = heads["n_user"].tolist()
    return [framing.unpack_bits(host[b], n_user[b]) for b in range(codec.B)], cover


# ---------------------------------------------------------------- capacity control: T chosen per slice
def _auto_args(codec, tmax, max_entries: int = 256, in_place: bool = False) -> int:
    tmax = codec.tmax if tmax is None else tmax
    check_args_auto(scheme=codec.scheme, tmax=tmax, gate=codec.gate, H=codec.H, W=codec.W, maxval=codec.maxval,
                    max_entries=max_entries, in_place=in_place)
    return int(tmax)


def embed_auto(codec, covers, payloads, *, tmax=None, stego=None, packed=None, checksum=False, max_entries: int = 256,
               check: bool = True):
    from . import checksum as _ck
    from .codec import _stream, _torch
    from .pee_checks import check_buffers
    torch = _torch()
    if checksum not in (False, True):
        raise ValueError("embed_blind_auto takes checksum=True or False (the header holds the cover's CRC-32 alone)")
    tmax = _auto_args(codec, tmax, max_entries)
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  covers=covers, stego=stego, packed=packed)
    _auto_args(codec, tmax, max_entries, in_place=stego is not None and stego.data_ptr() == covers.data_ptr())
    words, lengths, lens_t = packed if packed is not None else codec.pack_payloads(payloads)
    n_max = max([int(n) for n in lengths] + [0])
    if n_max > 64 * int(words.shape[1]):
        raise ValueError(f"a payload of {n_max} bits does not fit the packed rows' {64 * int(words.shape[1])}")
    pw = row_words(n_max, max_entries)
    crc = _ck.crc32_slices(covers) if checksum else None   # queued first, as embed_blind does
    if stego is None:
        stego = torch.empty_like(covers)
    ws = _workspace(codec, pw, max_entries, tmax)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    ts = torch.empty((codec.B,), dtype=torch.int32, device=codec.device)
    lm = torch.empty((codec.B, codec.lm_words), dtype=torch.int64, device=codec.device)
    meta = torch.empty((codec.B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=codec.device)
    P = _params_auto(codec, pw)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_embed_auto(
        C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), int(words.shape[1]), lens_t.data_ptr(),
        None if crc is None else crc.data_ptr(), tmax, int(max_entries), info.data_ptr(), ts.data_ptr(), meta.data_ptr(),
        lm.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_embed_auto"))
    out = info[:, :len(INFO_FIELDS)]
    if check:
        raise_status(out[:, 0].cpu().tolist(), "embed_blind_auto")   # one read-back
    return stego, out, ts


def capacity_curve(codec, covers, tmax=None, max_entries: int = 256):
    from .codec import _stream, _torch
    torch = _torch()
    tmax = _auto_args(codec, tmax, max_entries)
    codec._check_buffers(covers=covers)
    pw = row_words(0, max_entries)
    ws = _workspace(codec, pw, max_entries, tmax)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    ts = torch.empty((codec.B,), dtype=torch.int32, device=codec.device)
    curve = torch.empty((codec.B, tmax), dtype=torch.int32, device=codec.device)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_plan_auto(
        C.byref(_params_auto(codec, pw)), covers.data_ptr(), None, tmax, int(max_entries), info.data_ptr(), ts.data_ptr(),
        curve.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_plan_auto"))
    return curve


# ---------------------------------------------------------------- keyed: nonce and tag ride in the stego
def embed_keyed(codec, covers, payloads, *, key, nonce=None, index0: int = 0, tmax=None, stego=None, packed=None,
                max_entries: int = 256, check: bool = True):
    from . import aead as _aead
    from .codec import _stream, _torch
    from .pee_checks import check_buffers
    torch = _torch()
    if key is None:
        raise ValueError("embed_blind_keyed takes key= (32 bytes); embed_blind is the unkeyed call")
    key, nonce, index0 = _aead.check_call(key, nonce, index0, codec.B)   # judged before anything is queued
    auto = tmax is not None

    def rules(in_place=False):
        if auto:
            return _auto_args(codec, tmax, max_entries, in_place)
        _codec_args(codec, max_entries, in_place)
        return 0
    tmax = rules()
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  covers=covers, stego=stego, packed=packed)
    rules(in_place=stego is not None and stego.data_ptr() == covers.data_ptr())
    words, lengths, lens_t = packed if packed is not None else codec.pack_payloads(payloads)
    n_max = max([int(n) for n in lengths] + [0])
    if n_max > 64 * int(words.shape[1]):
        raise ValueError(f"a payload of {n_max} bits does not fit the packed rows' {64 * int(words.shape[1])}")
    pw = row_words(n_max + KEYED_FRAME_BITS, max_entries)
    lib = _lib.load()
    ctx = _aead.upload_ctx(key, nonce, codec.device)
    ct = _aead.chacha20_rows(ctx, words, lens_t, index0)          # into a new buffer: packed= rows are not modified
    tag = _aead.poly1305_tags(ctx, covers, ct, lens_t, index0)    # PeeCodec.embed(key=)'s tag of (cover, ciphertext)
    frames = torch.empty((codec.B, _lib.BLIND_FRAME_WORDS), dtype=torch.int32, device=codec.device)
    _lib.check(lib.codec_pee_blind_frames(ctx.data_ptr(), codec.B, index0, tag.data_ptr(), frames.data_ptr(), _stream()),
               "codec_pee_blind_frames")
    if stego is None:
        stego = torch.empty_like(covers)
    ws = _workspace(codec, pw, max_entries, tmax)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    ts = torch.empty((codec.B,), dtype=torch.int32, device=codec.device) if auto else \
        torch.full((codec.B,), codec.T, dtype=torch.int32, device=codec.device)
    lm = torch.empty((codec.B, codec.lm_words), dtype=torch.int64, device=codec.device)
    meta = torch.empty((codec.B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=codec.device)
    P = _params_auto(codec, pw) if auto else codec._params(pw)
    _guarded(codec, ws, pw, lambda: _lib.check(lib.codec_pee_blind_embed_keyed(
        C.byref(P), covers.data_ptr(), stego.data_ptr(), frames.data_ptr(), ct.data_ptr(), int(ct.shape[1]),
        lens_t.data_ptr(), tmax, int(max_entries), info.data_ptr(), ts.data_ptr() if auto else None, meta.data_ptr(),
        lm.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_embed_keyed"))
    out = info[:, :len(INFO_FIELDS)]
    if check:
        raise_status(out[:, 0].cpu().tolist(), "embed_blind_keyed")   # one read-back
    return stego, out, ts


def decode_keyed(codec, stego, key, *, cover=None, verify=True):
    from . import aead as _aead, checksum as _ck, framing
    from .codec import _stream, _torch
    torch = _torch()
    key = _aead.check_key(key)
    mode = _ck.verify_mode(verify)   # 'require' is satisfied by the tag every keyed slice carries
    hdr, heads = _headers(codec, stego, cover, keyed=True)
    words, cover, ws, pw = _extract(codec, stego, hdr, heads, cover)
    B = codec.B
    n_ct = (heads["n_user"] - KEYED_FRAME_BITS).tolist()
    cw = max(1, (max(n_ct) + 63) // 64)
    n12 = torch.empty((B, 3), dtype=torch.int32, device=codec.device)
    want = torch.empty((B, _aead.TAG_WORDS), dtype=torch.int32, device=codec.device)
    ct = torch.empty((B, cw), dtype=torch.int64, device=codec.device)
    ct_len = torch.empty((B,), dtype=torch.int32, device=codec.device)
    _lib.check(_lib.load().codec_pee_blind_unframe(B, words.data_ptr(), int(words.shape[1]), hdr.data_ptr(), n12.data_ptr(),
                                                   want.data_ptr(), ct.data_ptr(), cw, ct_len.data_ptr(), _stream()),
               "codec_pee_blind_unframe")
    ctx = _aead.upload_ctx(key, bytes(_aead.NONCE_BYTES), codec.device)   # the key alone: every slice brings its nonce
    if mode is None:
        pt, ok = _aead.chacha20_rows_n(ctx, n12, ct, ct_len), None
    else:   # the tag of (restored cover, ciphertext) compared and the rows released on the device
        got = _aead.poly1305_tags_n(ctx, n12, cover, ct, ct_len)
        pt, ok = _aead.release_n(ctx, n12, got, want, ct, ct_len)
    flag = _lookback_flag(codec, ws, pw)
    parts = [pt.reshape(-1)] + ([ok.to(torch.int64)] if ok is not None else []) + \
        ([flag.to(torch.int64)] if flag is not None else [])
    host = torch.cat(parts).cpu().numpy()   # the final read-back: rows, ok and the flag
    rows = host[:B * cw].reshape(B, cw)
    if flag is not None and int(host[-1]) != 0:
        _raise_lookback(codec, ws, pw)
    if ok is not None:
        bad = [b for b in range(B) if not int(host[B * cw + b])]
        if bad:
            raise _ck.IntegrityError(
                f"keyed blind MED-PEE decode: authentication failed in slices {bad} (Poly1305 tag mismatch: wrong key, or "
                "cover / payload / nonce / tag altered)", slices=bad, keyed=True, rows=rows)
    return [framing.unpack_bits(rows[b], n_ct[b]) for b in range(B)], cover


# ---------------------------------------------------------------- gated: (T, gate) chosen per slice
def gate_index(gate) -> int:
    """The ladder index of a gate value; ValueError naming the ladder for any other value."""
    if isinstance(gate, (bool, str)) or gate is None or gate != int(gate) or int(gate) not in GATES:
        raise ValueError(f"gated blind MED-PEE takes gate='auto' or a value of the ladder {GATES} "
                         f"(the header carries its index), got {gate!r}")
    return GATES.index(int(gate))


def check_args_gated(*, scheme: int, tmax, T=None, gate="auto", H: int, W: int, maxval: int, max_entries: int = 256,
                     roi=None, key=None, in_place: bool = False):
    """The argument rules of the gated blind calls, as ValueError before anything is queued, in
    check_args_auto's order with the gated calls' own T and gate in their places: scheme, tmax, T
    (None, or an integer in 1..tmax), gate ("auto" or a ladder value), roi / key, the shape, maxval,
    max_entries, in place.  Returns (t_fixed, j_fixed) as the library takes them (0 / -1: free)."""
    if int(scheme) == 1 and (isinstance(tmax, (bool, str)) or int(tmax) != tmax or not 1 <= int(tmax) <= TMAX):
        raise ValueError(f"gated blind MED-PEE chooses T in 1..tmax with tmax an integer in 1..{TMAX}, got {tmax!r}")
    t_fixed = 0
    if int(scheme) == 1 and T is not None:
        if isinstance(T, (bool, str)) or int(T) != T or not 1 <= int(T) <= int(tmax):
            raise ValueError(f"gated blind MED-PEE takes T=None or an integer in 1..tmax = {int(tmax)}, got {T!r}")
        t_fixed = int(T)
    j_fixed = -1 if int(scheme) != 1 or (isinstance(gate, str) and gate == "auto") else gate_index(gate)
    check_args(scheme=scheme, T=1, gate=None, H=H, W=W, maxval=maxval, max_entries=max_entries, roi=roi, key=key,
               in_place=in_place)
    return t_fixed, j_fixed


def _gated_args(codec, tmax, T, gate, max_entries: int = 256, in_place: bool = False):
    tmax = GATED_TMAX_DEFAULT if tmax is None else tmax
    t_fixed, j_fixed = check_args_gated(scheme=codec.scheme, tmax=tmax, T=T, gate=gate, H=codec.H, W=codec.W,
                                        maxval=codec.maxval, max_entries=max_entries, in_place=in_place)
    return int(tmax), t_fixed, j_fixed


def _workspace_gated(codec, pw: int, max_entries: int, tmax: int):
    """_workspace for the gated calls: the table of every (T, gate class) behind the blind workspace."""
    from collections import OrderedDict
    from .codec import _stream, _torch
    cache = codec.__dict__.setdefault("_ws_blind", OrderedDict())
    key = (int(pw), int(max_entries), int(tmax), "gated")
    if key not in cache:
        P = _params_auto(codec, pw)
        n = int(_lib.load().codec_pee_blind_gate_workspace_bytes(C.byref(P), int(tmax), int(max_entries)))
        if n == 0:
            _lib.check(-1, "codec_pee_blind_gate_workspace_bytes")
        ws = _torch().empty(n, dtype=_torch().uint8, device=codec.device)
        _lib.check(_lib.load().codec_pee_reset(C.byref(P), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_reset")
        cache[key] = ws
        while len(cache) > 4:
            cache.popitem(last=False)
    cache.move_to_end(key)
    return cache[key]


def embed_gated(codec, covers, payloads, *, gate="auto", T=None, tmax=None, stego=None, packed=None, checksum=False,
                max_entries: int = 256, check: bool = True):
    from . import checksum as _ck
    from .codec import _stream, _torch
    from .pee_checks import check_buffers
    torch = _torch()
    if checksum not in (False, True):
        raise ValueError("embed_blind_gated takes checksum=True or False (the header holds the cover's CRC-32 alone)")
    tmax, t_fixed, j_fixed = _gated_args(codec, tmax, T, gate, max_entries)
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  covers=covers, stego=stego, packed=packed)
    _gated_args(codec, tmax, T, gate, max_entries, in_place=stego is not None and stego.data_ptr() == covers.data_ptr())
    words, lengths, lens_t = packed if packed is not None else codec.pack_payloads(payloads)
    n_max = max([int(n) for n in lengths] + [0])
    if n_max > 64 * int(words.shape[1]):
        raise ValueError(f"a payload of {n_max} bits does not fit the packed rows' {64 * int(words.shape[1])}")
    pw = row_words(n_max, max_entries)
    crc = _ck.crc32_slices(covers) if checksum else None   # queued first, as embed_blind does
    if stego is None:
        stego = torch.empty_like(covers)
    ws = _workspace_gated(codec, pw, max_entries, tmax)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    ts = torch.empty((codec.B,), dtype=torch.int32, device=codec.device)
    gs = torch.empty((codec.B,), dtype=torch.int32, device=codec.device)
    lm = torch.empty((codec.B, codec.lm_words), dtype=torch.int64, device=codec.device)
    meta = torch.empty((codec.B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=codec.device)
    P = _params_auto(codec, pw)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_embed_gate(
        C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), int(words.shape[1]), lens_t.data_ptr(),
        None if crc is None else crc.data_ptr(), tmax, t_fixed, j_fixed, int(max_entries), info.data_ptr(), ts.data_ptr(),
        gs.data_ptr(), meta.data_ptr(), lm.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_embed_gate"))
    out = info[:, :len(INFO_FIELDS)]
    if check:
        raise_status(out[:, 0].cpu().tolist(), "embed_blind_gated")   # one read-back
    return stego, out, ts, gs


def capacity_gated(codec, covers, tmax=None, max_entries: int = 256):
    from .codec import _stream, _torch
    torch = _torch()
    tmax, _t, _j = _gated_args(codec, tmax, None, "auto", max_entries)
    codec._check_buffers(covers=covers)
    pw = row_words(0, max_entries)
    ws = _workspace_gated(codec, pw, max_entries, tmax)
    info = torch.empty((codec.B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    ts = torch.empty((codec.B,), dtype=torch.int32, device=codec.device)
    gs = torch.empty((codec.B,), dtype=torch.int32, device=codec.device)
    curve = torch.empty((codec.B, tmax, len(GATES)), dtype=torch.int32, device=codec.device)
    _guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_plan_gate(
        C.byref(_params_auto(codec, pw)), covers.data_ptr(), None, tmax, 0, -1, int(max_entries), info.data_ptr(),
        ts.data_ptr(), gs.data_ptr(), curve.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_plan_gate"))
    return curve

"""Blind volume payloads (include/codec_tcc_blind_vol.h): one bitstream planned on the
device across a stack of blind MED-PEE stegos, each of which carries a 192-bit frame naming its
place in the stream, so that the pixels alone decode it -- in any slice order, with unmarked slices
among them, and naming the stream bits of slices that are absent.

    stego, info, ts = codec.embed_blind_volume(covers, "one record for the series", tmax=8)
    bits, covers = other_codec.decode_blind_volume(stego[perm])

tests/pee_blind_volume_spec.py is the specification.  check_args, stream_crc and missing_ranges
are pure host code: no GPU, no library load.
"""
from __future__ import annotations

import ctypes as C
import secrets
import zlib
from typing import Dict, List, Tuple

import numpy as np

from . import _lib, blind as _blind

FLAG_VOLUME = _lib.BLIND_FLAG_VOLUME
FRAME_BITS = _lib.BVOL_FRAME_BITS
FRAME_WORDS = _lib.BVOL_FRAME_WORDS
FRAME_CRC = _lib.BVOL_FRAME_CRC
MAX_B = _lib.BVOL_MAX_B
NMAX = 2 ** 31 - 1
SKIPPED = _lib.BLIND_SKIPPED
PLAN_FIELDS = ("status", "T", "capacity", "capacity_max", "carriers", "N", "policy", "B")
ORDER_TEXT = {1: "no slice carries a volume frame", 2: "the slices belong to different volumes",
              3: "two slices claim one place in the stream (a duplicated or overlapping carrier, or a share out of range)",
              4: "stream bits are missing"}


def check_args(*, scheme: int, tmax, gate, B: int, H: int, W: int, maxval: int, nbits: int, policy: str = "even",
               max_entries: int = 256, roi=None, key=None, in_place: bool = False, volume_id=None) -> None:
    """The argument rules of embed_blind_volume, as ValueError before anything is queued: those of
    embed_blind_auto (blind.check_args_auto, in its order), then policy, B <= 65535, the candidates'
    product, N in 1..2^31 - 1 and volume_id in 0..2^32 - 1."""
    _blind.check_args_auto(scheme=scheme, tmax=tmax, gate=gate, H=H, W=W, maxval=maxval, max_entries=max_entries, roi=roi,
                           key=key, in_place=in_place)
    if policy not in _lib.VOL_POLICIES:
        raise ValueError(f"policy must be one of {sorted(_lib.VOL_POLICIES)}, got {policy!r}")
    if not 1 <= int(B) <= MAX_B:
        raise ValueError(f"a blind volume holds 1..{MAX_B} slices (the frame's 16 bits), got B = {int(B)}")
    if int(B) * (int(H) // 2) * (int(W) // 2) > NMAX:
        raise ValueError("B * (H // 2) * (W // 2) candidates exceed 2^31 - 1")
    if not 1 <= int(nbits) <= NMAX:
        raise ValueError(f"a blind volume payload holds 1 .. 2^31 - 1 bits, got N = {int(nbits)}")
    if volume_id is not None and (isinstance(volume_id, bool) or int(volume_id) != volume_id
                                  or not 0 <= int(volume_id) <= 0xFFFFFFFF):
        raise ValueError(f"volume_id must be None or an integer in 0..2^32 - 1, got {volume_id!r}")


def stream_crc(bits) -> int:
    """zlib CRC-32 of the stream's ceil(N / 8) bytes, LSB first, pad bits zero."""
    return zlib.crc32(np.packbits(np.asarray(bits, dtype=np.uint8).ravel(), bitorder="little").tobytes()) & 0xFFFFFFFF


def missing_ranges(table, N: int) -> List[Tuple[int, int]]:
    """The maximal ranges [lo, hi) of [0, N) that no carrier covers; table: rows (index, off, n, took)."""
    out, at = [], 0
    for _i, off, n, took in sorted(tuple(int(v) for v in r) for r in table):
        if not took:
            continue
        if off > at:
            out.append((at, off))
        at = max(at, off + n)
    if at < int(N):
        out.append((at, int(N)))
    return out


def _workspace(codec, pw: int, max_entries: int, tmax: int):
    from collections import OrderedDict
    from .codec import _stream, _torch
    cache = codec.__dict__.setdefault("_ws_bvol", OrderedDict())
    key = (int(pw), int(max_entries), int(tmax))
    if key not in cache:
        P = _blind._params_auto(codec, pw)
        n = int(_lib.load().codec_pee_blind_volume_workspace_bytes(C.byref(P), int(tmax), int(max_entries)))
        if n == 0:
            _lib.check(-1, "codec_pee_blind_volume_workspace_bytes")
        ws = _torch().empty(n, dtype=_torch().uint8, device=codec.device)
        _lib.check(_lib.load().codec_pee_reset(C.byref(P), ws.data_ptr(), ws.numel(), _stream()), "codec_pee_reset")
        cache[key] = ws
        while len(cache) > 4:
            cache.popitem(last=False)
    cache.move_to_end(key)
    return cache[key]


def embed(codec, covers, payload, *, volume_id=None, policy: str = "even", tmax=None, checksum=False,
          max_entries: int = 256, stego=None, check: bool = True, packed=None, key=None):
    from . import checksum as _ck, framing
    from .codec import _stream, _torch
    from .pee_checks import check_buffers
    torch = _torch()
    if checksum not in (False, True):
        raise ValueError("embed_blind_volume takes checksum=True or False")
    tmax = codec.tmax if tmax is None else tmax
    bits = framing.to_bits(payload) if packed is None else None
    N = int(bits.size) if packed is None else int(packed[1])

    def rules(in_place=False):
        check_args(scheme=codec.scheme, tmax=tmax, gate=codec.gate, B=codec.B, H=codec.H, W=codec.W, maxval=codec.maxval,
                   nbits=N, policy=policy, max_entries=max_entries, key=key, in_place=in_place, volume_id=volume_id)
    rules()
    tmax = int(tmax)
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  covers=covers, stego=stego)
    rules(in_place=stego is not None and stego.data_ptr() == covers.data_ptr())
    if packed is not None:
        if checksum:
            raise ValueError("packed= streams carry no stream CRC (the host does not see the bits): pass checksum=False")
        words = packed[0]
        if not isinstance(words, torch.Tensor) or words.device != covers.device or words.element_size() != 8 \
                or words.numel() < (N + 63) // 64 or not words.is_contiguous():
            raise ValueError("the packed stream (packed[0]) must hold ceil(bits / 64) contiguous 64-bit words on the device")
    else:
        words = torch.from_numpy(framing.pack_bits([bits])[0].reshape(-1)).to(codec.device)
    vid = secrets.randbits(32) if volume_id is None else int(volume_id)
    crc = stream_crc(bits) if checksum else 0
    nc = (codec.H // 2) * (codec.W // 2)
    pw = max(4, _blind.row_words(FRAME_BITS + min(N, nc), max_entries))
    cover_crc = _ck.crc32_slices(covers) if checksum else None   # queued first, as embed_blind does
    if stego is None:
        stego = torch.empty_like(covers)
    B = codec.B
    ws = _workspace(codec, pw, max_entries, tmax)
    side = torch.empty((B * (2 + FRAME_WORDS) + _lib.BVOL_INFO_WORDS,), dtype=torch.int32, device=codec.device)
    n, off = side[:B], side[B:2 * B]
    frames = side[2 * B:2 * B + FRAME_WORDS * B].view(B, FRAME_WORDS)
    vinfo = side[2 * B + FRAME_WORDS * B:]
    sinfo = torch.empty((B, _lib.BLIND_INFO_WORDS), dtype=torch.int32, device=codec.device)
    ts = torch.empty((B,), dtype=torch.int32, device=codec.device)
    lm = torch.empty((B, codec.lm_words), dtype=torch.int64, device=codec.device)
    meta = torch.empty((B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=codec.device)
    P = _blind._params_auto(codec, pw)
    _blind._guarded(codec, ws, pw, lambda: _lib.check(_lib.load().codec_pee_blind_volume_embed(
        C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), N, _lib.VOL_POLICIES[policy], tmax,
        int(max_entries), vid, int(bool(checksum)), crc, None if cover_crc is None else cover_crc.data_ptr(), n.data_ptr(),
        off.data_ptr(), frames.data_ptr(), vinfo.data_ptr(), sinfo.data_ptr(), ts.data_ptr(), meta.data_ptr(), lm.data_ptr(),
        ws.data_ptr(), ws.numel(), _stream()), "codec_pee_blind_volume_embed"))
    info = {"volume": vinfo, "volume_id": vid, "n": n, "off": off, "frames": frames,
            "slices": sinfo[:, :len(_blind.INFO_FIELDS)]}
    if check:
        v = vinfo.cpu().tolist()   # one read-back
        if v[0] != 0:
            raise ValueError(f"embed_blind_volume: N = {N} bits exceed the stack's capacity S(tmax) = {v[3]} at tmax = {tmax} "
                             "(a blind volume is refused, never truncated; the stego is the covers)")
    return stego, info, ts


def _classify(hdr_host: np.ndarray, H: int, W: int, nbytes: int):
    """(carriers, heads for all B slices): a slice without the magic is no carrier (a record that
    copies through); one with the magic must carry a valid volume header."""
    w = hdr_host.astype(np.int64) & 0xFFFFFFFF
    B = w.shape[0]
    carrier = w[:, 0] == _blind.MAGIC
    idx = np.flatnonzero(carrier)
    heads: Dict[str, np.ndarray] = {k: np.zeros(B, np.int64) for k in ("T", "flags", "maxval", "n_user", "E", "end", "crc",
                                                                       "n_side", "L")}
    heads["rect"] = np.zeros((B, 4), np.int64)
    heads["T"][:] = 1
    heads["end"][:] = -1
    if idx.size:
        try:
            got = _blind.parse_headers(w[idx], H, W, nbytes, volume=True)
        except ValueError as e:   # the slices named by their place in the stack
            raise ValueError(f"decode_blind_volume: among the slices {idx.tolist()} that carry the magic: {e}") from None
        for k, v in got.items():
            heads[k][idx] = v
    return carrier, heads


def decode(codec, stego, *, cover=None, verify=True, partial: bool = False):
    from . import checksum as _ck, framing
    from .codec import _stream, _torch
    from .pee_checks import check_buffers, check_records
    torch = _torch()
    mode = _ck.verify_mode(verify)
    if codec.scheme != 1:
        raise ValueError("blind MED-PEE is scheme 1's")
    if codec.B > MAX_B:
        raise ValueError(f"a blind volume holds at most {MAX_B} slices, got B = {codec.B}")
    if codec.H > _blind.MAX_DIM or codec.W > _blind.MAX_DIM or codec.H * codec.W < _blind.HDR_BITS:
        raise ValueError(f"a {codec.H} x {codec.W} slice carries no blind MED-PEE header")
    check_buffers(codec.device, codec.B, codec.H, codec.W, codec.bytes, lm_words=codec.lm_words, scheme=1,
                  stego=stego, cover=cover)
    if cover is not None and cover.data_ptr() == stego.data_ptr():
        raise ValueError("blind MED-PEE decodes out of place only: pass a cover buffer other than the stego")
    B = codec.B
    lib = _lib.load()
    hdr = torch.empty((B, 8), dtype=torch.int32, device=codec.device)
    _lib.check(lib.codec_pee_blind_headers(C.byref(codec._params(1)), stego.data_ptr(), hdr.data_ptr(), _stream()),
               "codec_pee_blind_headers")
    carrier, heads = _classify(hdr.cpu().numpy().view(np.uint32), codec.H, codec.W, codec.bytes)   # the one read-back before
    if not carrier.any():
        raise ValueError(f"decode_blind_volume: {ORDER_TEXT[1]}")
    heads["maxval"][~carrier] = codec.maxval
    has_crc = carrier & ((heads["flags"] & _blind.FLAG_CRC) != 0)
    if mode == "require" and not has_crc[carrier].all():
        raise _ck.IntegrityError("blind volume decode: verify='require' and slices "
                                 f"{np.flatnonzero(carrier & ~has_crc).tolist()} carry no cover checksum")
    pw = max(4, int((heads["L"].max() + 63) // 64))
    uw = max(3, int((heads["n_user"].max() + 63) // 64))
    raw = _blind.records_bytes(heads, codec.H, codec.W)
    check_records([_lib.PeeMeta.from_buffer_copy(raw, b * _lib.PEE_META_BYTES) for b in range(B)], codec.H, codec.W,
                  scheme=1, payload_words=pw, lm_words=codec.lm_words, bytes=codec.bytes)
    up = np.concatenate([np.frombuffer(raw, dtype=np.uint8), (~carrier).astype("<i4").view(np.uint8)])
    dev = torch.from_numpy(up.copy()).to(codec.device)   # records and skip marks: one upload
    meta = dev[:B * _lib.PEE_META_BYTES].view(B, _lib.PEE_META_BYTES)
    skip = dev[B * _lib.PEE_META_BYTES:].view(torch.int32)
    if cover is None:
        cover = torch.empty_like(stego)
    sw = max(1, int(((heads["n_user"][carrier] - FRAME_BITS).sum() + 63) // 64))
    rows = torch.empty((B, uw), dtype=torch.int64, device=codec.device)
    out = torch.empty((sw + (_lib.BVOL_INFO_WORDS + 4 * B + 1) // 2,), dtype=torch.int64, device=codec.device)
    stream = out[:sw]
    tail = out[sw:].view(torch.int32)
    oinfo, table = tail[:_lib.BVOL_INFO_WORDS], tail[_lib.BVOL_INFO_WORDS:_lib.BVOL_INFO_WORDS + 4 * B]
    ws = _workspace(codec, pw, 0, 1)
    P = _blind._params_auto(codec, pw)   # T is only range-checked: the records carry each slice's
    _blind._guarded(codec, ws, pw, lambda: _lib.check(lib.codec_pee_blind_volume_extract(
        C.byref(P), stego.data_ptr(), hdr.data_ptr(), meta.data_ptr(), skip.data_ptr(), cover.data_ptr(), rows.data_ptr(),
        uw, stream.data_ptr(), sw, oinfo.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
        "codec_pee_blind_volume_extract"))
    flagged = np.flatnonzero(has_crc).tolist()
    got = _ck.crc32_slices(cover) if mode is not None and flagged else None
    host = out.cpu().numpy()   # stream, order info and table: one read-back
    flag = _blind._lookback_flag(codec, ws, pw)
    if flag is not None and int(flag.item()) != 0:
        _blind._raise_lookback(codec, ws, pw)
    tail_h = host[sw:].view(np.int32)
    oi = tail_h[:_lib.BVOL_INFO_WORDS].astype(np.int64) & 0xFFFFFFFF
    tab = tail_h[_lib.BVOL_INFO_WORDS:_lib.BVOL_INFO_WORDS + 4 * B].reshape(B, 4)[carrier]
    status, N = int(oi[0]), int(oi[2])
    missing = missing_ranges(tab, N) if status in (0, 4) else []
    if status not in (0, 4) or (status == 4 and not partial):
        raise ValueError(f"decode_blind_volume: {ORDER_TEXT.get(status, 'status %d' % status)}"
                         + (f"; missing stream bits {missing} of {N}" if status == 4 else "")
                         + f" (carriers at stack positions {np.flatnonzero(carrier).tolist()[:16]})")
    if got is not None:
        from . import pee_verify as _pv
        bad = set(_pv.cover_mismatches(got, heads["crc"].tolist(), B))
        _ck.raise_mismatch([b for b in flagged if b in bad], [], "blind volume decode")
    words_h = host[:sw]
    if status == 4 and (N + 63) // 64 > sw:   # the absent slices' bits read 0: the stream at its full length
        full = torch.empty(((N + 63) // 64,), dtype=torch.int64, device=codec.device)
        _lib.check(lib.codec_pee_blind_volume_gather(C.byref(P), rows.data_ptr(), uw, oinfo.data_ptr(), full.data_ptr(),
                                                     int(full.numel()), ws.data_ptr(), ws.numel(), _stream()),
                   "codec_pee_blind_volume_gather")
        words_h = full.cpu().numpy()
    bits = framing.unpack_bits(words_h, N)
    if mode is not None and status == 0 and int(oi[3]) & FRAME_CRC and stream_crc(bits) != int(oi[7]):
        raise _ck.IntegrityError(f"blind volume decode: the stream's CRC-32 {stream_crc(bits):#010x} is not the frames' "
                                 f"{int(oi[7]):#010x} (a share was altered)")
    return (bits, cover, missing) if partial else (bits, cover)

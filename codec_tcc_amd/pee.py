"""MED-predictor prediction-error expansion (PEE) on the MI355X -- the algorithm the north
star names.  The reference contains no PEE code; the scheme is specified in
oracle/pee_cpu.py (parity unpinned) and summarised in include/codec_tcc.h.

    codec = PeeCodec(B, H, W, dtype="uint16", T=2)
    enc = codec.embed(covers, payloads)          # stego, location map, per-slice meta
    bits, cover = codec.decode(enc)

Scheme 2 (PeeCodec(..., scheme=2), oracle/pee_cpu.py "Scheme 2"): four sublattice passes on
the running image, about four times the capacity at one T; enc.meta / enc.lm then hold one
record / map per pass ([4, B, ...], pass-major).  With T="auto" each slice's workgroup tries
T = tmin .. tmax inside one launch and keeps the first T that holds the payload
(include/codec_tcc_ext.h, codec_pee_multi_embed_auto).

Volume payloads (scheme 1; include/codec_tcc_vol.h): one bitstream across the whole stack,

    vol = codec.embed_volume(covers, payload, policy="even")   # device plan + cut + embed
    bits, covers = codec.decode_volume(vol)

with the per-slice bit counts and T chosen on the device from the capacity curves.  With
embed_volume(..., gate="auto") (or an integer gate; include/codec_tcc_gvol.h) the plan is over
(T, G): the smoothness gate of PeeCodec(gate=...) chosen for the volume and again per slice.

Regions of interest (scheme 1; include/codec_tcc_roi.h, roi.py): codec.embed(..., roi=) takes a
per-slice pixel rectangle that the stego leaves bit-identical to the cover; the records carry
it, decode() needs no configuration.

Keyed embedding (include/codec_tcc_aead.h, aead.py): codec.embed(..., key=, nonce=)
encrypts the payload rows with ChaCha20 and tags (cover, ciphertext) with Poly1305 per slice;
codec.decode(enc, key=) authenticates the restored cover and the extracted rows on the device
before any plaintext leaves it.  codec.embed_blind_keyed / decode_blind_keyed (blind.py)
do the same for a blind stego, which then carries its nonce and tag itself.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, aead as _aead, blind as _blind, checksum as _ck, framing, pee_verify as _pv, roi as _roi
from .codec import _elem_bytes, _require_gpu, _stream, _torch
from .pee_checks import (VOLUME_NMAX, _bad_device, _bad_overlap, _bad_pixels, _bad_side,  # noqa: F401 (re-exported)
                         _check_multi_args, _dense, _on_device, _pix_dtypes, check_buffers, check_gate_args,
                         check_gvol_args, check_records, check_roi_args, check_volume_args, lattice_geometry,
                         make_record)


@dataclass
class PeeEncoded:
    stego: object      # torch [B,H,W]
    lm: object         # torch.int64 [B, lm_words]: overflow location map, bit k = candidate k
    meta: object       # torch.uint8 [B, sizeof(codec_pee_meta)]
    lengths: List[int]
    payload_words: int
    config: dict = field(default_factory=dict)   # the PeeCodec's T / tmax / maxval (decode())
    scheme: int = 1                              # 2: four sublattice passes (meta / lm per pass)
    cover_crc: object = None                     # torch.int32 [B] (device): CRC-32 of each cover (checksum=True)
    payload_crc: Optional[List[int]] = None      # CRC-32 of each slice's payload bits (checksum.payload_crc32)
    cover_tile_crc: object = None                # torch.int32 [B, nty, ntx] (device): CRC-32 per tile (checksum="tiles")
    tile: Optional[Tuple[int, int]] = None       # the table's (th, tw)
    tag: object = None                           # torch.int32 [B, 4] (device): Poly1305 tag per slice (embed(key=))
    nonce: Optional[bytes] = None                # the 8-byte nonce of a keyed embedding
    index0: int = 0                              # global index of slice 0 (the nonce's first word is index0 + b)

    def records(self) -> List[_lib.PeeMeta]:
        """Scheme 1: one record per slice.  Scheme 2: 4 * B records, pass-major."""
        raw = self.meta.detach().cpu().contiguous().numpy().tobytes()
        n = len(raw) // _lib.PEE_META_BYTES
        return [_lib.PeeMeta.from_buffer_copy(raw, i * _lib.PEE_META_BYTES) for i in range(n)]

    @property
    def roi(self) -> List[Tuple[int, int, int, int]]:
        """Scheme 1: the per-slice rectangles (y0, x0, y1, x1) read from the records ((0, 0, 0, 0):
        none).  One read-back."""
        if self.scheme != 1:
            raise ValueError("regions of interest are scheme 1's")
        return _roi.records_roi(self.records())

    def pass_records(self) -> List[List[_lib.PeeMeta]]:
        """Scheme 2: records[p][b] of pass p (scheme 1: one pass)."""
        recs = self.records()
        n = len(self.lengths)
        return [recs[i:i + n] for i in range(0, len(recs), n)]

    def embedded(self) -> List[int]:
        """Payload bits embedded per slice (scheme 2: the passes' sum)."""
        if self.scheme == 1:
            return [int(min(r.L, r.capacity)) if r.status == 1 else int(r.L) for r in self.records()]
        prs = self.pass_records()   # one read-back
        return [sum(int(pr[b].L) for pr in prs) for b in range(len(self.lengths))]


_TILE_UNSET = object()   # embed(tile=) not given: checksum.TILE_DEFAULT (a ROI call with tiles insists on one)


@dataclass
class PeeVolume:
    """One bitstream embedded across a slice stack (PeeCodec.embed_volume).  enc is an ordinary
    scheme-1 PeeEncoded -- every slice stays decodable and storable by the per-slice code;
    enc.lengths holds the slices' bit counts once they were read back (check=True, or
    decode_volume), zeros before."""
    enc: PeeEncoded
    total_bits: int                   # the stream's bits (what was asked for)
    policy: str
    plan: object                      # torch.int32 [3 B + 1] (device): n[B], T[B], off[B + 1]; gated: + g[B]
    info: object                      # torch.int32 [8] (device): codec_pee_volume_info; gated: [10], codec_pee_gvol_info
    payload_crc: Optional[int] = None   # CRC-32 of the whole stream (checksum.payload_crc32)
    embedded_bits: Optional[int] = None  # info.total, once read back (check=True): < total_bits when truncated
    gate: object = None               # embed_volume's gate= (None: an ungated volume)
    tag: object = None                # torch.int32 [1, 4] (device): the stream's Poly1305 tag (embed_volume(key=))

    def plan_host(self) -> dict:
        """n, t, off (numpy) and the info record's fields: one read-back.  A gated volume adds
        g (the slices' gate values) and gate (the volume's G*, or the fixed gate)."""
        torch = _torch()
        B = len(self.enc.lengths)
        both = torch.cat([self.plan.reshape(-1), self.info.reshape(-1)]).cpu().numpy()
        np_ = self.plan.numel()
        return _plan_dict(both[:np_], both[np_:], B, gated=self.gate is not None)


def _plan_dict(plan, info, B: int, gated: bool = False) -> dict:
    rec = _lib.PeeGvolInfo if gated else _lib.PeeVolumeInfo
    i = rec.from_buffer_copy(np.ascontiguousarray(info, dtype=np.int32).tobytes())
    d = {"n": plan[:B].copy(), "t": plan[B:2 * B].copy(), "off": plan[2 * B:3 * B + 1].copy(),
         "status": int(i.status), "T": int(i.T), "total": int(i.total), "requested": int(i.requested),
         "capacity": int(i.capacity), "policy": {v: k for k, v in _lib.VOL_POLICIES.items()}[int(i.policy)]}
    if gated:
        d["g"], d["gate"] = plan[3 * B + 1:4 * B + 1].copy(), int(i.gate)
    return d


class PeeCodec:
    def __init__(self, batch: int, height: int, width: int, dtype="uint16", *, T=2, tmin: int = 1, tmax: int = 16,
                 maxval: Optional[int] = None, device=None, scheme: int = 1, gate=None):
        """gate (scheme 1; include/codec_tcc_gate.h): None, a smoothness gate G in 0..65535, or
        "auto".  A candidate whose MED neighbours W, N, NW span more than G (max - min) is left
        alone: it is not shifted, flags nothing and carries nothing, and the decoder, reading the
        same never-modified neighbours, skips it too -- the shifts of busy regions, most of the
        distortion on real images, are gone at no cost in side information.  "auto" picks, per
        slice on the device, the (T, G) of the 16-gate ladder with the least modelled distortion
        per embedded bit among those that hold the payload (with an integer T: the best G for
        that T); an integer gate with T="auto" picks the smallest T that holds the payload under
        that gate.  meta.reserved[1] = G + 1 records the choice, g_slices holds it per slice
        (t_slices the T).  Needs tmax <= 16 and at most 2^26 candidates per slice.
        T: the expansion threshold for every slice, or "auto" -- capacity control: each
        slice gets the smallest T <= tmax whose capacity holds its payload (meta.T records
        the choice, t_slices holds it per slice).  Scheme 1 reads it off the cover's capacity
        curve (codec_pee_capacity, one extra read-only pass); scheme 2's capacity depends on
        the bits already embedded, so its workgroup tries T = tmin, tmin + 1, ... tmax inside
        one launch (codec_pee_multi_embed_auto; out of place only; a slice no T fits is the
        truncated T = tmax embedding).  tmin: scheme 2 only.
        scheme: 1 = the (odd, odd) lattice in one pass; 2 = four sublattice passes."""
        if scheme not in (1, 2):
            raise ValueError("scheme must be 1 or 2")
        if scheme == 1 and int(tmin) != 1:
            raise ValueError("tmin is scheme 2's (scheme 1's capacity control starts at T = 1)")
        self.scheme = int(scheme)
        check_gate_args(gate, T, tmax, (height // 2) * (width // 2), scheme)
        self.gate = gate if gate is None or isinstance(gate, str) else int(gate)
        _require_gpu()
        torch = _torch()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type == "cuda" and self.device.index is None:   # "cuda": the current card, as tensors name it
            self.device = torch.device("cuda", torch.cuda.current_device())
        nbytes = 2 if "16" in str(dtype) else 1
        if str(dtype) not in ("uint16", "torch.uint16", "uint8", "torch.uint8"):
            raise ValueError("A imagem deve ser uint8 ou uint16.")
        vmax = 65535 if nbytes == 2 else 255
        self.B, self.H, self.W, self.bytes = int(batch), int(height), int(width), nbytes
        self.auto = isinstance(T, str)
        if self.auto and T != "auto":
            raise ValueError("T must be an integer >= 1 or 'auto'")
        self.T = 1 if self.auto else int(T)
        if not 1 <= int(tmax) <= 64:
            raise ValueError("tmax must be in 1..64")
        self.tmax = int(tmax)
        if not 1 <= int(tmin) <= self.tmax:
            raise ValueError("tmin must be in 1..tmax")
        self.tmin = int(tmin)
        self.maxval = vmax if maxval is None else int(maxval)
        self.nc = (self.H // 2) * (self.W // 2)
        self.lm_words = max(1, (self.nc + 63) // 64)
        self.config = dict(method="pee", T="auto" if self.auto else self.T, tmax=self.tmax, maxval=self.maxval,
                           dtype="uint16" if nbytes == 2 else "uint8", scheme=self.scheme)
        if self.scheme == 2:
            self.config["tmin"] = self.tmin
        if self.gate is not None:
            self.config["gate"] = self.gate
        P = self._params(1)
        # a gated codec's workspace is the codec_pee one with the capacity table's bins behind
        # it (every codec_pee call accepts it)
        if self.gate is not None:
            ws = _lib.load().codec_pee_gate_workspace_bytes(C.byref(P), self.tmax)
        else:
            ws = _lib.load().codec_pee_workspace_bytes(C.byref(P))
        if ws == 0:
            _lib.check(-1, "codec_pee_workspace_bytes")
        # zeroed by the reset below (codec_pee_reset: the whole workspace, the cumulative
        # look-back diagnostics included -- codec_pee_diag_offset)
        self.workspace = torch.empty(int(ws), dtype=torch.uint8, device=self.device)
        self.t_slices = torch.empty(self.B, dtype=torch.int32, device=self.device) \
            if self.auto or self.gate is not None else None
        self.g_slices = torch.empty(self.B, dtype=torch.int32, device=self.device) if self.gate is not None else None
        if self.gate is not None and not self.auto:
            self.t_slices.fill_(self.T)
        if isinstance(self.gate, int):
            self.g_slices.fill_(self.gate)
        # register the fresh workspace with the library: an allocation at an address
        # an earlier workspace used would otherwise inherit that one's call-to-call state record
        self.reset()

    def reset(self):
        """Re-zero the workspace (codec_pee_reset, on the current stream): the state small
        out-of-place batches carry from call to call starts afresh, and the cumulative
        diagnostics read zero.  Called automatically after a failed call (include/codec_tcc.h,
        codec_pee_workspace_bytes: recovery rules)."""
        _lib.check(_lib.load().codec_pee_reset(C.byref(self._params(1)), self.workspace.data_ptr(),
                                               self.workspace.numel(), _stream()), "codec_pee_reset")

    def _guarded(self, fn, *args):
        """Run one workspace call; on any exception re-zero the workspace, then re-raise."""
        try:
            return fn(*args)
        except BaseException:
            try:
                self.reset()
            except Exception:   # the original error is the one to report
                pass
            raise

    def _embed_status(self, recs):
        """An embed's records once read back: a status other than 0 / 1 is no capacity overflow, so
        the workspace starts clean; a look-back that gave up is the RuntimeError."""
        if any(r.status not in (0, 1) for r in recs):
            self.reset()
        _raise_lookback(recs)

    def _check_buffers(self, **tensors):
        """check_buffers() with this codec's device, shape and scheme."""
        check_buffers(self.device, self.B, self.H, self.W, self.bytes, lm_words=self.lm_words, scheme=self.scheme,
                      **tensors)

    def _params(self, payload_words: int) -> _lib.PeeParams:
        return _lib.PeeParams(B=self.B, H=self.H, W=self.W, bytes=self.bytes, T=self.T, maxval=self.maxval,
                              payload_words=int(payload_words), lm_words=self.lm_words)

    def pack_payloads(self, payloads):
        torch = _torch()
        bits = [framing.to_bits(p) for p in payloads]
        if len(bits) != self.B:
            raise ValueError("one payload per slice is required")
        packed, lengths = framing.pack_bits(bits)
        return (torch.from_numpy(packed).to(self.device), lengths,
                torch.tensor(lengths, dtype=torch.int32, device=self.device))

    def pack_roi(self, roi):
        """roi.PackedRoi for embed(..., roi=): the rectangles judged (roi.normalize_roi: None, one
        4-tuple for every slice, or [B, 4]) and uploaded once, for calls that must not read back
        or upload (a captured graph), as pack_payloads is for the payloads."""
        if isinstance(roi, _roi.PackedRoi):
            return roi
        host = check_roi_args(roi, self.B, self.H, self.W, scheme=self.scheme, T="auto" if self.auto else self.T,
                              tmax=self.tmax, gate=self.gate)
        if host is None:
            return None
        return _roi.PackedRoi(host, _torch().from_numpy(host).to(self.device))

    def _roi_slices(self):
        """(t_slices, g_slices) of a ROI call: the codec's own where it is gated, else tensors kept
        beside them (g = 65535: no gate asked for)."""
        torch = _torch()
        if self.gate is not None:
            return self.t_slices, self.g_slices
        g = self.__dict__.get("_roi_g")
        if g is None:
            g = self._roi_g = torch.full((self.B,), _lib.GATE_MAX, dtype=torch.int32, device=self.device)
            self._roi_t = self.t_slices if self.auto else torch.full((self.B,), self.T, dtype=torch.int32,
                                                                      device=self.device)
        return self._roi_t, g

    def _table_workspace(self, tmax: int):
        """The workspace of a codec_pee_gate_capacity call: the codec's own when it is a gated
        one's, else a table-only one kept beside it (the call uses the tail alone)."""
        torch = _torch()
        need = int(_lib.load().codec_pee_gate_workspace_bytes(C.byref(self._params(1)), int(tmax)))
        if need == 0:
            _lib.check(-1, "codec_pee_gate_workspace_bytes")
        if self.workspace.numel() >= need:
            return self.workspace
        ws = self.__dict__.get("_gate_ws")
        if ws is None or ws.numel() < need:
            ws = self._gate_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def gate_table(self, covers, tmax: Optional[int] = None, gate: Optional[int] = None, roi=None):
        """(n, hs): the gated capacity table of every slice as int32 device tensors [B, 16] and
        [B, tmax, 16] (include/codec_tcc_gate.h): n[b, j] = candidates of roughness class j
        (first j with D <= _lib.GATES[j]), hs[b, u, j] = those whose expansion is safe and whose
        folded error is u.  hs.cumsum(1).cumsum(2)[b, T - 1, j] is the capacity at
        (T, GATES[j]).  gate: the two-class table of one gate instead (class 0 = D <= gate).
        roi: the slices' rectangles (embed's roi=): protected candidates fall into no class."""
        torch = _torch()
        if self.scheme != 1:
            raise ValueError("the smoothness gate is scheme 1's")
        tmax = self.tmax if tmax is None else int(tmax)
        check_gate_args(0 if gate is None else gate, 1, tmax, self.nc)
        self._check_buffers(covers=covers)
        rects = self.pack_roi(roi)
        n = torch.empty((self.B, 16), dtype=torch.int32, device=self.device)
        hs = torch.empty((self.B, tmax, 16), dtype=torch.int32, device=self.device)
        ws = self._table_workspace(tmax)
        # the two entries differ by the rectangles' pointer alone
        what, extra = ("codec_pee_gate_capacity", ()) if rects is None else \
            ("codec_pee_roi_capacity", (rects.device.data_ptr(),))
        _lib.check(getattr(_lib.load(), what)(
            C.byref(self._params(1)), covers.data_ptr(), tmax, 0, -1 if gate is None else int(gate), None, *extra,
            n.data_ptr(), hs.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), _stream()), what)
        return n, hs

    def capacity(self, covers, tmax: Optional[int] = None, gate: Optional[int] = None, roi=None):
        """int32 [B, tmax] device tensor: exact capacity of each slice at T = 1..tmax.
        Bounded by the candidate lattice: at most (H // 2) * (W // 2) bits per slice -- a
        quarter of the pixels; the other three quarters are the MED context, never modified.
        gate: the capacities under that smoothness gate (active candidates only).
        roi: the capacities outside the slices' rectangles (embed's roi=; with or without a gate)."""
        torch = _torch()
        tmax = self.tmax if tmax is None else int(tmax)
        if gate is not None or roi is not None:
            _n, hs = self.gate_table(covers, tmax, _lib.GATE_MAX if gate is None else gate, roi=roi)
            return hs[:, :, 0].cumsum(1).to(torch.int32)
        self._check_buffers(covers=covers)
        caps = torch.empty((self.B, tmax), dtype=torch.int32, device=self.device)
        self._guarded(lambda: _lib.check(_lib.load().codec_pee_capacity(
            C.byref(self._params(1)), covers.data_ptr(), tmax, None, caps.data_ptr(), None, self.workspace.data_ptr(),
            self.workspace.numel(), _stream()), "codec_pee_capacity"))
        return caps

    def embed(self, covers, payloads, *, stego=None, lm=None, meta=None, packed=None, check: bool = True,
              checksum=False, tile=_TILE_UNSET, roi=None, key=None, nonce=None, index0: int = 0) -> PeeEncoded:
        """cover -> stego + location map + per-slice meta.  check=True (default) reads the
        per-slice status back (one sync) and raises RuntimeError if an in-place look-back
        gave up (CODEC_PEE_ELOOKBACK: the slice is not a valid stego); check=False keeps
        the call asynchronous (benchmarks) -- inspect enc.records() afterwards.
        checksum=True: enc.cover_crc = crc32_slices(covers), launched on the same stream BEFORE
        the embed (so an in-place embed checksums the cover, not the stego), and
        enc.payload_crc from the bits on the host (None with caller-packed `packed=` payloads:
        the bits are not here); decode(enc) then verifies both.
        checksum="tiles": everything checksum=True records, and enc.cover_tile_crc =
        crc32_tiles(covers, tile) (int32 [B, nty, ntx]; tile: an int or (th, tw), 4..1024), queued
        before the embed too; a decode whose cover check fails then names the tiles that differ
        (IntegrityError.tiles).
        roi (scheme 1; include/codec_tcc_roi.h): None, one rectangle (y0, x0, y1, x1)
        for every slice, a [B, 4] array / list / device tensor, or pack_roi()'s result.  The stego
        is bit-identical to the cover on every pixel of a slice's rectangle: candidates inside it
        are left alone and count nowhere, exactly as those a smoothness gate rejects.  The records
        carry the rectangle (enc.roi) and decode() follows them.  With T="auto" / gate="auto" the
        capacity table leaves the protected candidates out.  checksum=True composes (the CRCs are
        the cover's); checksum="tiles" does with an explicit tile=.
        tile: the default is a private "not given" marker that stands for checksum.TILE_DEFAULT (64),
        exactly as before; it exists so that a call with roi= and checksum="tiles" can tell whether
        the tile was chosen by the caller.
        key (32 bytes; include/codec_tcc_aead.h): the payload rows are encrypted with
        ChaCha20 into a buffer of the codec's (caller-packed `packed=` rows are not modified) and
        enc.tag = the Poly1305 tag of (cover, ciphertext) per slice, queued BEFORE the embed (so an
        in-place embed authenticates the cover, not the stego); the embed then runs unchanged on the
        encrypted rows.  nonce: 8 bytes, fresh from os.urandom when None -- never reuse one under
        a key; index0: the global index of slice 0 (a rank of a sharded stack passes its first
        slice's), slices index0 .. index0 + B - 1 all < 2^31.  enc.payload_crc is None (the tag
        covers the payload).  A slice truncated by capacity (record status 1) is reported as
        today and its tag will not verify.  key=None: nothing of this runs."""
        torch = _torch()
        key, nonce, index0 = _aead.check_call(key, nonce, index0, self.B)   # judged before anything is queued
        checksum, tiled = _ck.checksum_mode(checksum)
        tile_given = tile is not _TILE_UNSET
        if not tile_given:
            tile = _ck.TILE_DEFAULT
        tile = _ck.check_tile_args(tile) if tiled else None
        if roi is not None:   # judged (and uploaded) before anything is queued, the checksum launches included
            if tiled and not tile_given:
                check_roi_args((0, 0, 0, 0), self.B, self.H, self.W, scheme=self.scheme, tiled=True, tile_given=False)
            roi = self.pack_roi(roi)
        # every buffer of the call, before anything is queued (the checksum launch included)
        check_buffers(self.device, self.B, self.H, self.W, self.bytes, lm_words=self.lm_words, scheme=self.scheme,
                      covers=covers, stego=stego, lm=lm, meta=meta, packed=packed)
        if self.scheme == 2 and self.auto and stego is not None and _same_storage(covers, stego):
            raise ValueError("scheme 2 with T='auto' embeds out of place only (a failed trial is undone from "
                             "the cover): pass a stego buffer other than the covers")
        cover_crc = payload_crc = tile_crc = None
        if checksum:
            cover_crc = _ck.crc32_slices(covers)   # queued first: the host work below runs beside it
            if tiled:
                tile_crc = _ck.crc32_tiles(covers, tile)
            if packed is None and key is None:   # pack here (what _embed would do) and checksum the packed rows
                bits = [framing.to_bits(p) for p in payloads]
                if len(bits) != self.B:
                    raise ValueError("one payload per slice is required")
                rows, lengths = framing.pack_bits(bits)
                payload_crc = [_ck.payload_crc32_packed(rows[b], lengths[b]) for b in range(self.B)]
                packed = (torch.from_numpy(rows).to(self.device), lengths,
                          torch.tensor(lengths, dtype=torch.int32, device=self.device))
        tag = None
        if key is not None:
            words, lengths, lens_t = packed if packed is not None else self.pack_payloads(payloads)
            ctx = _aead.upload_ctx(key, nonce, self.device)
            ct = _aead.chacha20_rows(ctx, words, lens_t, index0)
            tag = _aead.poly1305_tags(ctx, covers, ct, lens_t, index0)
            packed = (ct, lengths, lens_t)
        enc = self._embed(covers, payloads, stego, lm, meta, packed, check, roi)
        if tag is not None:
            enc.tag, enc.nonce, enc.index0 = tag, nonce, index0
        enc.cover_crc, enc.payload_crc = cover_crc, payload_crc
        enc.cover_tile_crc, enc.tile = tile_crc, tile
        return enc

    def _embed(self, covers, payloads, stego, lm, meta, packed, check, roi=None) -> PeeEncoded:
        torch = _torch()
        words, lengths, lens_t = packed if packed is not None else self.pack_payloads(payloads)
        rects = self.pack_roi(roi) if roi is not None else None
        if stego is None:
            stego = torch.empty_like(covers)
        if self.scheme == 2:
            return self._embed_multi(covers, words, lengths, lens_t, stego, lm, meta, check)
        if lm is None:
            lm = torch.empty((self.B, self.lm_words), dtype=torch.int64, device=self.device)
        if meta is None:
            meta = torch.empty((self.B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=self.device)
        P = self._params(words.shape[1])
        lib = _lib.load()

        def launch_roi():
            # the gated routes with the slices' rectangles (include/codec_tcc_roi.h)
            rp = rects.device.data_ptr()
            ts, gs = self._roi_slices()
            if self.gate is not None and (self.auto or self.gate == "auto"):
                tmax = self.tmax if self.auto else self.T
                _lib.check(lib.codec_pee_roi_embed_auto(
                    C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), lens_t.data_ptr(), tmax,
                    0 if self.auto else self.T, -1 if self.gate == "auto" else self.gate, rp, ts.data_ptr(), gs.data_ptr(),
                    meta.data_ptr(), lm.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), _stream()),
                    "codec_pee_roi_embed_auto")
                return
            if self.auto:   # an ungated codec: the smallest T that holds the payload outside the rectangle,
                # from the table pass on the table workspace (as gate_table), then the embed on the codec's own
                tws = self._table_workspace(self.tmax)
                _lib.check(lib.codec_pee_roi_capacity(
                    C.byref(P), covers.data_ptr(), self.tmax, 0, _lib.GATE_MAX, lens_t.data_ptr(), rp, None, None,
                    ts.data_ptr(), gs.data_ptr(), None, tws.data_ptr(), tws.numel(), _stream()), "codec_pee_roi_capacity")
            _lib.check(lib.codec_pee_roi_embed(
                C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), lens_t.data_ptr(), ts.data_ptr(),
                gs.data_ptr(), rp, meta.data_ptr(), lm.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(),
                _stream()), "codec_pee_roi_embed")

        def launch():
            if rects is not None:
                return launch_roi()
            if self.gate is not None and (self.auto or self.gate == "auto"):
                # the gated table, the (T, G) selection and the embed queued on this stream
                tmax = self.tmax if self.auto else self.T
                _lib.check(lib.codec_pee_gate_embed_auto(
                    C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), lens_t.data_ptr(), tmax,
                    0 if self.auto else self.T, -1 if self.gate == "auto" else self.gate, self.t_slices.data_ptr(),
                    self.g_slices.data_ptr(), meta.data_ptr(), lm.data_ptr(), self.workspace.data_ptr(),
                    self.workspace.numel(), _stream()), "codec_pee_gate_embed_auto")
            elif self.gate is not None:   # T and G given: t_slices / g_slices were filled at construction
                _lib.check(lib.codec_pee_gate_embed(
                    C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), lens_t.data_ptr(),
                    self.t_slices.data_ptr(), self.g_slices.data_ptr(), meta.data_ptr(), lm.data_ptr(),
                    self.workspace.data_ptr(), self.workspace.numel(), _stream()), "codec_pee_gate_embed")
            elif self.auto:   # capacity control: per-slice T on the device (fused into the embed
                # launch where it runs slice-serial, else one read-only capacity pass first)
                _lib.check(lib.codec_pee_embed_auto(C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(),
                                                    lens_t.data_ptr(), self.tmax, self.t_slices.data_ptr(),
                                                    meta.data_ptr(), lm.data_ptr(), self.workspace.data_ptr(),
                                                    self.workspace.numel(), _stream()), "codec_pee_embed_auto")
            else:
                _lib.check(lib.codec_pee_embed_ts(C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(),
                                                  lens_t.data_ptr(), None, meta.data_ptr(), lm.data_ptr(),
                                                  self.workspace.data_ptr(), self.workspace.numel(), _stream()),
                           "codec_pee_embed")
        self._guarded(launch)
        enc = PeeEncoded(stego=stego, lm=lm, meta=meta, lengths=list(lengths), payload_words=int(words.shape[1]),
                         config=self.config)
        if check:
            self._embed_status(enc.records())
        return enc

    def _embed_multi(self, covers, words, lengths, lens_t, stego, lm, meta, check):
        """Scheme 2: passes 0..3 in one library call (codec_pee_multi_embed: one slice-serial
        launch after scheme 1's pass 0 on chip-filling batches, per-pass tile launches
        otherwise); pass 0 copies cover -> stego, the others run in place.  T="auto":
        codec_pee_multi_embed_auto, one launch that scans T per slice (out of place only)."""
        torch = _torch()
        if lm is None:
            lm = torch.empty((4, self.B, self.lm_words), dtype=torch.int64, device=self.device)
        if meta is None:
            meta = torch.empty((4, self.B, _lib.PEE_META_BYTES), dtype=torch.uint8, device=self.device)
        _check_multi_args(self.B, self.lm_words, meta, lm)
        P = self._params(words.shape[1])
        lib = _lib.load()
        if self.auto:
            self._guarded(lambda: _lib.check(lib.codec_pee_multi_embed_auto(
                C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), lens_t.data_ptr(), self.tmin,
                self.tmax, self.t_slices.data_ptr(), meta.data_ptr(), lm.data_ptr(), self.workspace.data_ptr(),
                self.workspace.numel(), _stream()), "codec_pee_multi_embed_auto"))
        else:
            self._guarded(lambda: _lib.check(lib.codec_pee_multi_embed(
                C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), lens_t.data_ptr(), meta.data_ptr(),
                lm.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), _stream()), "codec_pee_multi_embed"))
        enc = PeeEncoded(stego=stego, lm=lm, meta=meta, lengths=list(lengths), payload_words=int(words.shape[1]),
                         config=self.config, scheme=2)
        if check:   # pass 0 in place runs scheme 1's look-back embed
            self._embed_status(enc.pass_records()[0])
        return enc

    def extract(self, stego, meta, lm, *, payload_words: int, cover=None, payload=None, gated: Optional[bool] = None,
                roi: bool = False):
        """gated: decode through codec_pee_gate_extract, which takes each record's gate
        (reserved[1]; it reads ungated records too).  None: this codec's own setting; decode()
        passes what the records say.  roi=True: through codec_pee_roi_extract, which takes the
        gate and the rectangle (reserved[0], reserved[2]) from each record and reads every other
        scheme-1 record too; decode() passes what the records say."""
        torch = _torch()
        check_buffers(self.device, self.B, self.H, self.W, self.bytes, lm_words=self.lm_words, scheme=self.scheme,
                      stego=stego, cover=cover, lm=lm, meta=meta, payload=payload, payload_words=payload_words)
        if cover is None:
            cover = torch.empty_like(stego)
        if payload is None:
            payload = torch.empty((self.B, int(payload_words)), dtype=torch.int64, device=self.device)
        if self.scheme == 2:
            return self._extract_multi(stego, meta, lm, payload_words, cover, payload)
        P = self._params(payload_words)
        gated = self.gate is not None if gated is None else bool(gated)
        fn, what = (_lib.load().codec_pee_gate_extract, "codec_pee_gate_extract") if gated else \
            (_lib.load().codec_pee_extract, "codec_pee_extract")
        if roi:
            _roi.check_roi_shape(self.H, self.W)
            fn, what = _lib.load().codec_pee_roi_extract, "codec_pee_roi_extract"
        self._guarded(lambda: _lib.check(fn(
            C.byref(P), stego.data_ptr(), meta.data_ptr(), lm.data_ptr(), cover.data_ptr(), payload.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel(), _stream()), what))
        return payload, cover

    def _extract_multi(self, stego, meta, lm, payload_words, cover, payload):
        """Scheme 2: passes 3..0 in one library call (codec_pee_multi_extract; the first copies
        stego -> cover, the others run in place; payload written whole)."""
        _check_multi_args(self.B, self.lm_words, meta, lm, payload=payload, payload_words=payload_words)
        P = self._params(payload_words)
        lib = _lib.load()
        self._guarded(lambda: _lib.check(lib.codec_pee_multi_extract(
            C.byref(P), stego.data_ptr(), meta.data_ptr(), lm.data_ptr(), cover.data_ptr(), payload.data_ptr(),
            self.workspace.data_ptr(), self.workspace.numel(), _stream()), "codec_pee_multi_extract"))
        return payload, cover

    def lookback_failed(self, payload_words: int = 1) -> bool:
        """True when the last in-place extract's look-back gave up (its payload is invalid)."""
        off = int(_lib.load().codec_pee_extract_flag_offset(C.byref(self._params(payload_words))))
        return bool(off) and int(self.workspace[off:off + 4].view(_torch().int32).item()) != 0

    def diagnostics(self, payload_words: int = 1) -> dict:
        """Cumulative look-back counters since construction (codec_pee_diag_offset)."""
        off = int(_lib.load().codec_pee_diag_offset(C.byref(self._params(payload_words))))
        v = self.workspace[off:off + 16].view(_torch().int32).cpu().tolist()
        return {"embed_fallback_chunks": v[0], "extract_fallback_chunks": v[1],
                "embed_unrecovered_chunks": v[2], "extract_unrecovered_chunks": v[3]}

    def repaired(self, payload_words: int = 1) -> int:
        """Chunks whose look-back fell back to counting predecessors from pixels (exact)."""
        d = self.diagnostics(payload_words)
        return d["embed_fallback_chunks"] + d["extract_fallback_chunks"]

    def _t_text(self) -> str:
        gate = "" if self.gate is None else f", gate={self.gate}"
        return f"T={'auto, tmax=%d' % self.tmax if self.auto else self.T}{gate}"

    def _check(self, enc: PeeEncoded, recs, lengths=None):
        """check_records() on records already read back (decode: no extra sync)."""
        check_records(recs, self.H, self.W, scheme=self.scheme, payload_words=enc.payload_words,
                      lm_words=self.lm_words, bytes=self.bytes, lengths=lengths)

    def verify_tiles(self, enc: PeeEncoded, cover) -> np.ndarray:
        """Host bool [B, nty, ntx]: the tiles of `cover` (a restored [B,H,W] stack on the GPU) whose
        CRC-32 differs from the table enc carries (embed(..., checksum="tiles")).  Never raises
        IntegrityError: for callers that decode with verify=False and want the map beside the
        data.  ValueError for an encoding without a table, or a table of another grid, dtype or
        device."""
        if enc.cover_tile_crc is None or enc.tile is None:
            raise ValueError("the encoding carries no tile table (embed with checksum='tiles')")
        self._check_buffers(covers=cover)
        maps = _ck.tile_mismatch_maps(cover, enc.cover_tile_crc, enc.tile, range(self.B))
        return np.stack([maps[b] for b in range(self.B)])

    def _keyed_check(self, enc: PeeEncoded, key):
        """decode's key= against the encoding, before any launch; the checked key or None."""
        key = _pv.check_key(getattr(enc, "tag", None) is not None, key)
        if key is not None:
            _aead.check_nonce(enc.nonce)
            _aead.check_index(enc.index0, self.B)
            _aead._check_tags(enc.tag, self.B, self.device, "enc.tag")
        return key

    def decode(self, enc: PeeEncoded, verify=True, key=None):
        """(list of 0/1 bit vectors, restored cover tensor); raises if a slice overflowed, and
        ValueError for records that are not an embed's (check_records).
        verify=True: the checksums enc carries (embed(..., checksum=True)) are compared with the
        restored cover's (one crc32_slices launch behind the extract) and the payloads';
        IntegrityError names the slices and which of cover / payload failed.  verify=False
        skips it; verify='require' also raises when a checksum is absent.
        key: required for a keyed embedding (embed(key=); ValueError before any launch when it is
        missing, or given for an unkeyed one).  Order: extract, Poly1305 over the restored cover
        and the extracted rows, the release (tags compared on the device), then the one read-back,
        which also brings ok.  IntegrityError (.keyed = True, .slices) names the slices whose tag
        failed; their plaintext never reaches the host.  verify=False decrypts without the tag
        pass.  verify='require' is satisfied by the tag, which covers cover and payload."""
        mode = _ck.verify_mode(verify)
        key = self._keyed_check(enc, key)
        _pv.check_require(mode, key is not None, enc.cover_crc is not None, enc.payload_crc is not None)
        if enc.scheme != self.scheme:
            raise ValueError(f"a scheme-{enc.scheme} embedding given to a scheme-{self.scheme} codec")
        self._check_buffers(stego=enc.stego, lm=enc.lm, meta=enc.meta)   # before the records' read-back
        if self.scheme == 2:
            prs = enc.pass_records()   # one read-back serves the capacity test and the record check
            got = [sum(int(pr[b].L) for pr in prs) for b in range(len(enc.lengths))]
            short = [i for i, (g, n) in enumerate(zip(got, enc.lengths)) if g < n]
            if short:
                raise ValueError(f"payload exceeds PEE capacity in slices {short} (scheme 2, {self._t_text()})")
            self._check(enc, prs, enc.lengths)
            kw = {}
        else:
            recs = enc.records()
            _raise_lookback(recs)
            _raise_status(recs, self._t_text())
            self._check(enc, recs)
            # the gate is the records': a gated embedding decodes on any scheme-1 codec of the shape
            kw = dict(gated=any(int(r.reserved[1]) != 0 for r in recs), roi=any(int(r.reserved[2]) != 0 for r in recs))
        words, cover = self.extract(enc.stego, enc.meta, enc.lm, payload_words=enc.payload_words, **kw)
        # scheme 2's extract passes have no look-back (tile or slice-serial): no flag to read
        host, _total = _pv.after_extract(self, enc, cover, words, mode, key, lookback=self.scheme == 1)
        return [framing.unpack_bits(host[i], enc.lengths[i]) for i in range(self.B)], cover

    # ---- blind MED-PEE: the stego alone carries its map and record (include/codec_tcc_blind.h, blind.py)
    def embed_blind(self, covers, payloads, *, stego=None, packed=None, checksum=False, max_entries: int = 256,
                    check: bool = True):
        """(stego, info): every slice's stego carries its own header and location map in the LSBs
        of its last rows, so decode_blind(stego) needs nothing else.  info: int32
        [B, 6] on the device, per slice (status, n_user, E, n_side, end, region row); status 1: the
        payload and its 192 + 32 E side bits do not fit, 2: E > max_entries -- such a slice is
        copied through unchanged and carries no header.  Scheme 1 with a fixed T and no gate, out
        of place; row table, plan, splice, ROI embed and pack are queued on the current stream
        with no host round trip (capturable with packed= and check=False).
        checksum=True: crc32_slices(covers), queued first, goes into the header and decode_blind
        verifies it.  max_entries: the most location-map entries a slice may need (it sizes the
        payload rows).  check=True reads the statuses back (one sync) and raises ValueError naming
        the refused slices; check=False leaves them in info."""
        return _blind.embed(self, covers, payloads, stego=stego, packed=packed, checksum=checksum,
                            max_entries=max_entries, check=check)

    def decode_blind(self, stego, *, cover=None, verify=True):
        """(bits per slice, cover) of embed_blind's stegos, from the pixels alone: T, maxval, the
        lengths, the region and the map come from each slice's header, whatever this codec was
        built with (its shape and dtype are the stego's).  The headers are gathered and read back
        once; anything that is no header of such a slice is a ValueError naming the slices, before
        the extract is launched, and the rebuilt records pass check_records.  verify (True, False,
        'require'): a slice whose header carries the cover's CRC-32 and whose restored cover has
        another raises IntegrityError (.bad_cover), as decode(verify=True) does."""
        return _blind.decode(self, stego, cover=cover, verify=verify)

    def blind_capacity(self, covers, max_entries: int = 256):
        """int32 [B] device tensor: the most user bits embed_blind takes per slice at this codec's T
        (the plan rule of DESIGN §3k), -1 where not even the header fits."""
        return _blind.capacity(self, covers, max_entries)

    def embed_blind_auto(self, covers, payloads, *, tmax=None, stego=None, packed=None, checksum=False,
                         max_entries: int = 256, check: bool = True):
        """(stego, info, ts): embed_blind with T chosen per slice on the device (DESIGN §3l;
        include/codec_tcc_blind_auto.h): the smallest T in 1..tmax whose plan takes the slice's
        payload, so the least distortion that holds it.  ts: int32 [B] on the device, the chosen T,
        0 for a refused slice, whose info is the plan's at tmax.  tmax: 1..16, None: this codec's.
        The codec's own T is ignored (fixed or "auto"); every other rule of embed_blind holds, and
        decode_blind reads the stego as it is.  One pass over the covers fills the row table of
        every T; nothing is read back before the embed (capturable with packed= and check=False)."""
        return _blind.embed_auto(self, covers, payloads, tmax=tmax, stego=stego, packed=packed, checksum=checksum,
                                 max_entries=max_entries, check=check)

    def embed_blind_gated(self, covers, payloads, *, gate="auto", T=None, tmax=None, stego=None, packed=None,
                          checksum=False, max_entries: int = 256, check: bool = True):
        """(stego, info, ts, gs): embed_blind with the pair (T, gate) chosen per slice on the device
        (include/codec_tcc_blind_gate.h): over T in 1..tmax (None: 4) and the gates of the
        ladder _lib.GATES, the smallest T for which some gate has a plan, and at that T the smallest
        such gate; only candidates whose MED context is that flat are modified, and the gate rides
        in the slice's header, so decode_blind reads the stego as it is.  ts / gs: int32 [B] device
        tensors, the chosen T and gate (0 and -1: refused, the slice is copied through with no
        header).  T= (an integer in 1..tmax) or gate= (a ladder value; anything else is a ValueError
        naming the ladder) fixes one of the two, or both.  The codec's own T and gate are ignored;
        every other rule of embed_blind holds."""
        return _blind.embed_gated(self, covers, payloads, gate=gate, T=T, tmax=tmax, stego=stego, packed=packed,
                                  checksum=checksum, max_entries=max_entries, check=check)

    def blind_capacity_gated(self, covers, tmax=None, max_entries: int = 256):
        """int32 [B, tmax, 16] device tensor: the most user bits embed_blind_gated takes per slice at
        every (T in 1..tmax, gate _lib.GATES[j]), -1 where not even 0 bits fit (tmax None: 4)."""
        return _blind.capacity_gated(self, covers, tmax, max_entries)

    def embed_blind_keyed(self, covers, payloads, *, key, nonce=None, index0: int = 0, tmax=None, stego=None, packed=None,
                          max_entries: int = 256, check: bool = True):
        """(stego, info, ts): a blind stego that is confidential and authenticated under a 32-byte key
        (include/codec_tcc_blind_keyed.h).  Each slice's user bits are a 224-bit frame --
        nonce12 = LE32(index0 + b) || nonce, then the Poly1305 tag of (cover, ciphertext), the tag
        embed(key=) computes -- and the ChaCha20 ciphertext of its payload; header flag bit 1 marks it.
        info[:, 1] is the header's n_user, frame included.  tmax=None: the codec's fixed T (ts holds
        it); tmax in 1..16: T chosen per slice as embed_blind_auto does.  nonce: 8 bytes, drawn from
        os.urandom when None; never reuse one under a key.  Key, nonce, index and every rule of
        embed_blind are judged before anything is queued; the queue order is chacha20_rows,
        poly1305_tags, the frames, the embed, and check=False makes no host round trip.  There is no
        CRC beside the tag."""
        return _blind.embed_keyed(self, covers, payloads, key=key, nonce=nonce, index0=index0, tmax=tmax, stego=stego,
                                  packed=packed, max_entries=max_entries, check=check)

    def decode_blind_keyed(self, stego, key, *, cover=None, verify=True):
        """(bits per slice, cover) of embed_blind_keyed's stegos from the pixels and the key; the
        slices of a batch may come from different calls, each brings its nonce and index.  After the
        header read-back (ValueError naming the slices whose flags are not exactly 2 or whose n_user is
        below 224 -- an unkeyed stego is decode_blind's) everything runs on the device: extract,
        unframe, the tag of (restored cover, ciphertext), release.  IntegrityError(keyed=True,
        slices=...) names the slices whose tag fails; their plaintext never reaches the host (rows
        holds the device's zeros).  verify=False decrypts without the tag pass; 'require' is
        satisfied by the tag."""
        return _blind.decode_keyed(self, stego, key, cover=cover, verify=verify)

    # ---- blind volume payloads: one stream across self-contained stegos (include/codec_tcc_blind_vol.h)
    def embed_blind_volume(self, covers, payload, *, volume_id=None, policy: str = "even", tmax=None, checksum=False,
                           max_entries: int = 256, stego=None, check: bool = True, packed=None, key=None):
        """(stego, info, ts): one payload (str / bytes / 0-1 vector) embedded across the stack as blind
        stegos (blind_volume.py).  The device plans the shares (embed_volume's rule on the
        blind capacity curve less the 192 frame bits, policy "even" or "fill"), and every slice that
        takes bits carries a frame -- volume_id, its index, B, its offset, N, the stream's CRC -- before
        its share, so decode_blind_volume needs the pixels alone, in any order.  A slice that takes no
        bit is copied through (ts 0, info["slices"] status 3).  info: {"volume": int32 [8] device
        tensor (status, T*, S(T*), S(tmax), carriers, N, policy, B), "volume_id", "n", "off" (int32 [B]),
        "frames" (int32 [B, 6]), "slices" (int32 [B, 6], embed_blind's fields)}.  A payload beyond
        S(tmax) is refused, never truncated: the stego is the covers, and check=True (one read-back)
        raises ValueError with N and S(tmax).  volume_id=None draws 32 random bits.  checksum=True:
        the covers' CRC-32 in the headers and the stream's in the frames.  packed=(words, N): the
        stream already on the device (no upload; no stream CRC).  One pass over the covers, no host
        round trip, capturable with check=False.  key: must be None (a blind volume is unkeyed)."""
        from . import blind_volume as _bv
        return _bv.embed(self, covers, payload, volume_id=volume_id, policy=policy, tmax=tmax, checksum=checksum,
                         max_entries=max_entries, stego=stego, check=check, packed=packed, key=key)

    def decode_blind_volume(self, stego, *, cover=None, verify=True, partial: bool = False):
        """(bits, covers) of embed_blind_volume's stegos from the pixels alone, the slices in any
        order; slices without a blind header are tolerated and returned as they are.  ValueError
        when no slice carries a frame, volumes are mixed, a carrier is duplicated or stream bits are
        missing (the message names the ranges); a slice with a blind header that is no volume slice's
        is a ValueError too.  partial=True: missing bits read 0 and (bits, covers, missing) is
        returned, missing the list of uncovered ranges [lo, hi).  IntegrityError when a restored
        cover or the stream fails the CRC-32 it carries (verify as decode_blind's)."""
        from . import blind_volume as _bv
        return _bv.decode(self, stego, cover=cover, verify=verify, partial=partial)

    def blind_capacity_curve(self, covers, tmax=None, max_entries: int = 256):
        """int32 [B, tmax] device tensor: blind_capacity at every T in 1..tmax (None: this codec's
        tmax, at most 16), from one pass over the covers."""
        return _blind.capacity_curve(self, covers, tmax, max_entries)

    # ---- volume payloads: one bitstream across the stack (include/codec_tcc_vol.h)
    def _cached_workspace(self, fn: str, payload_words: int, tmax: int):
        """A workspace sized by the library's `fn` for this row pitch; the last few are kept, so a
        steady stream of equal-sized payloads allocates once per side."""
        key = (int(payload_words), int(tmax))
        cache = self.__dict__.setdefault("_ws_" + fn, OrderedDict())
        if key not in cache:
            n = int(getattr(_lib.load(), fn)(C.byref(self._params(payload_words)), tmax))
            if n == 0:
                _lib.check(-1, fn)
            cache[key] = _torch().empty(n, dtype=_torch().uint8, device=self.device)
            while len(cache) > 4:
                cache.popitem(last=False)
        cache.move_to_end(key)
        return cache[key]

    def _volume_workspace(self, payload_words: int, tmax: int):
        """The volume workspace (capacity curves, payload rows, offsets)."""
        return self._cached_workspace("codec_pee_volume_workspace_bytes", payload_words, tmax)

    def _gvol_workspace(self, payload_words: int, tmax: int):
        """The gated volume workspace (offsets, payload rows, the slices' tables)."""
        return self._cached_workspace("codec_pee_gvol_workspace_bytes", payload_words, tmax)

    def _side_words(self, gated: bool):
        """int32 words of the plan and of the info record in a volume's side buffer."""
        if gated:
            return 4 * self.B + 1, _lib.PEE_GVOL_INFO_BYTES // 4
        return 3 * self.B + 1, _lib.PEE_VOLUME_INFO_BYTES // 4

    def volume_buffers(self, gate: bool = False):
        """(lm, side) for embed_volume(..., buffers=): the location map and the one int32 buffer
        that holds records, plan and info, so that a caller (a captured graph) can preallocate.
        gate=True: the larger side buffer of a gated volume (the plan gains g[B], the info
        record is codec_pee_gvol_info)."""
        torch = _torch()
        lm = torch.empty((self.B, self.lm_words), dtype=torch.int64, device=self.device)
        side = torch.empty(self.B * _lib.PEE_META_BYTES // 4 + sum(self._side_words(bool(gate))),
                           dtype=torch.int32, device=self.device)
        return lm, side

    def pack_volume(self, payload):
        """(stream words on the device, bit count) for embed_volume(..., packed=): the upload a
        caller does once when the same call is captured into a graph."""
        bits = framing.to_bits(payload)
        check_volume_args((self.B, self.H, self.W), bits.size, "even", self.scheme)
        return _torch().from_numpy(framing.pack_bits([bits])[0].reshape(-1)).to(self.device), int(bits.size)

    def embed_volume(self, covers, payload, *, policy: str = "even", stego=None, check: bool = True,
                     checksum=False, buffers=None, packed=None, gate=None, tile=_ck.TILE_DEFAULT,
                     roi=None, key=None, nonce=None, index0: int = 0) -> "PeeVolume":
        """One payload (str / bytes / 0-1 vector, framing.to_bits) embedded across the whole
        stack: the device plans how many bits each slice takes and at which T (the rule of
        include/codec_tcc_vol.h: policy "even" spreads the bits in proportion to the slices'
        capacities at the smallest volume T that holds them, "fill" fills slices in order; each
        slice then gets the smallest T that holds its share), cuts the stream into payload rows
        and embeds them -- capacity pass, plan, cut and embed are queued on the current stream,
        no host round trip.  tmax is the codec's; the T given at construction is
        ignored here.  Scheme 1 only.
        gate: None (ungated, as ever), a smoothness gate 0..65535 or "auto" -- a gated volume
        (include/codec_tcc_gvol.h; the codec itself is built without gate=).  "auto": the device
        sums the slices' gated capacity tables, picks the volume's (T*, G*) by the per-slice
        selection rule, shares the bits by the capacities at that pair and lets every slice
        re-choose its own (T_b, G_b) for its share; an integer gate plans T alone under that
        gate.  The records carry the gates, so every slice still decodes on its own.  Needs
        tmax <= 16 and at most 2^26 candidates per slice; buffers: volume_buffers(gate=True).
        check=True (default): one read-back of records, plan and info fills enc.lengths and
        embedded_bits, raises RuntimeError if an in-place look-back gave up (the workspace is
        reset, as embed does); a payload beyond the volume's capacity at tmax is truncated to
        it (info status 1, embedded_bits < total_bits; every slice stays reversible).
        check=False keeps the call asynchronous.
        checksum=True: enc.cover_crc per slice as embed, plus one payload CRC over the whole
        stream (over the embedded prefix when check=True saw a truncation); decode_volume
        verifies both.  stego may be the covers (in place).  buffers: volume_buffers();
        packed: pack_volume()'s result instead of `payload` (no upload in the call; the payload
        CRC is then absent, as with embed's packed=).
        checksum="tiles": checksum=True plus enc.cover_tile_crc / enc.tile as embed records them;
        decode_volume then names the tiles of a cover that fails its check.
        roi: must be None -- volume payloads take no region of interest.
        key / nonce / index0: the whole stream is encrypted as one row at the reserved
        index 0x80000000 into a buffer of the codec's, every cover gets a tag with an empty
        ciphertext at index0 + b (enc.tag, queued before the embed), and after the embed the
        stream is tagged (vol.tag, empty associated data) over its first info.total bits, the
        length read on the device -- a truncated volume authenticates exactly the prefix it
        embedded.  The payload CRC is then absent (the tag covers the payload)."""
        torch = _torch()
        # judged before anything is queued (and, unkeyed, before the codec's shape is looked at)
        key, nonce, index0 = _aead.check_call(key, nonce, index0, self.B if key is not None else 1)
        if roi is not None:
            raise ValueError("volume payloads take no region of interest: the plan's capacities are the whole "
                             "slices' (DESIGN §3i); embed per slice with embed(..., roi=)")
        checksum, tiled = _ck.checksum_mode(checksum)
        tile = _ck.check_tile_args(tile) if tiled else None
        check_gvol_args(self.gate, gate, self.tmax, self.nc, self.scheme)
        gated = gate is not None
        self._check_buffers(covers=covers, stego=stego)
        bits = framing.to_bits(payload) if packed is None else None
        N = int(bits.size) if packed is None else int(packed[1])
        check_volume_args((self.B, self.H, self.W), N, policy, self.scheme)
        pw = max(1, min((N + 63) // 64, self.lm_words))
        nm = self.B * _lib.PEE_META_BYTES // 4
        npl, _ninfo = self._side_words(gated)
        # the caller's other buffers, judged like the pixels' before the upload and the checksum launch
        if packed is not None:
            if not _on_device(packed[0], self.device):
                _bad_device("packed[0]", packed[0], self.device)
            if packed[0].element_size() != 8 or packed[0].numel() < max(1, (N + 63) // 64) or not packed[0].is_contiguous():
                raise ValueError("the packed stream (packed[0]) must hold ceil(bits / 64) contiguous 64-bit words")
        if buffers is not None:
            lm, side = buffers
            if not _dense(lm, self.device, (self.B, self.lm_words), 8) or \
                    not _dense(side, self.device, (nm + npl + _ninfo,), 4):
                raise ValueError("buffers must be what volume_buffers() returns" + (" with gate=True" if gated else ""))
        words = packed[0] if packed is not None else \
            torch.from_numpy(framing.pack_bits([bits])[0].reshape(-1)).to(self.device)
        cover_crc = _ck.crc32_slices(covers) if checksum else None   # before an in-place embed
        tile_crc = _ck.crc32_tiles(covers, tile) if tiled else None
        ctx = cover_tag = None
        if key is not None:   # the stream encrypted into a new buffer, the covers tagged before the embed
            ctx = _aead.upload_ctx(key, nonce, self.device)
            words = _aead.chacha20_rows(ctx, words.reshape(1, -1), torch.tensor([N], dtype=torch.int32, device=self.device),
                                        _aead.STREAM_INDEX).reshape(-1)
            cover_tag = _aead.poly1305_tags(ctx, covers, index0=index0)
        if stego is None:
            stego = torch.empty_like(covers)
        if buffers is None:
            lm, side = self.volume_buffers(gated)
        meta = side[:nm].view(torch.uint8).view(self.B, _lib.PEE_META_BYTES)
        plan, info = side[nm:nm + npl], side[nm + npl:]
        P = self._params(pw)
        n_ptr = plan.data_ptr()
        if gated:   # table, plan over (T, G), cut and gated embed, queued on this stream
            gws, tws = self._gvol_workspace(pw, self.tmax), self._table_workspace(self.tmax)
            self._guarded(lambda: _lib.check(_lib.load().codec_pee_gvol_embed(
                C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), N, _lib.VOL_POLICIES[policy],
                self.tmax, -1 if gate == "auto" else int(gate), n_ptr, n_ptr + 4 * self.B, n_ptr + 4 * (3 * self.B + 1),
                n_ptr + 8 * self.B, info.data_ptr(), meta.data_ptr(), lm.data_ptr(), self.workspace.data_ptr(),
                self.workspace.numel(), tws.data_ptr(), tws.numel(), gws.data_ptr(), gws.numel(), _stream()),
                "codec_pee_gvol_embed"))
        else:
            vws = self._volume_workspace(pw, self.tmax)
            self._guarded(lambda: _lib.check(_lib.load().codec_pee_volume_embed(
                C.byref(P), covers.data_ptr(), stego.data_ptr(), words.data_ptr(), N, _lib.VOL_POLICIES[policy], self.tmax,
                n_ptr, n_ptr + 4 * self.B, n_ptr + 8 * self.B, info.data_ptr(), meta.data_ptr(), lm.data_ptr(),
                self.workspace.data_ptr(), self.workspace.numel(), vws.data_ptr(), vws.numel(), _stream()),
                "codec_pee_volume_embed"))
        config = dict(self.config, T="auto")
        if gated:
            config["gate"] = gate if isinstance(gate, str) else int(gate)
        enc = PeeEncoded(stego=stego, lm=lm, meta=meta, lengths=[0] * self.B, payload_words=pw,
                         config=config, cover_crc=cover_crc, cover_tile_crc=tile_crc, tile=tile)
        vol = PeeVolume(enc=enc, total_bits=N, policy=policy, plan=plan, info=info, gate=config.get("gate"),
                        payload_crc=_ck.payload_crc32(bits) if checksum and bits is not None and key is None else None)
        if key is not None:   # the stream's tag over info.total (word 2 of either info record), read on the device
            vol.tag = _aead.poly1305_tags(ctx, None, words.reshape(1, -1), info[2:3], _aead.STREAM_INDEX)
            enc.tag, enc.nonce, enc.index0 = cover_tag, nonce, index0
        if check:
            host = side.cpu().numpy()   # records, plan and info: one read-back
            raw = host[:nm].tobytes()
            self._embed_status([_lib.PeeMeta.from_buffer_copy(raw, i * _lib.PEE_META_BYTES) for i in range(self.B)])
            p = _plan_dict(host[nm:nm + npl], host[nm + npl:], self.B, gated)
            enc.lengths = [int(v) for v in p["n"]]
            vol.embedded_bits = p["total"]
            if checksum and bits is not None and key is None and p["total"] < N:
                vol.payload_crc = _ck.payload_crc32(bits[:p["total"]])
        return vol

    def decode_volume(self, vol: "PeeVolume", verify=True, key=None):
        """(bits, covers): the stream's embedded bits as one 0/1 vector (the first
        embedded_bits of a truncated volume) and the restored stack.  The records are read back
        and judged by check_records first; extract and the stream's reassembly are launches on
        the current stream, then one read-back of the stream.  verify as decode(): the cover
        CRCs per slice and the one payload CRC embed_volume(checksum=True) recorded.
        key: required for a keyed volume (embed_volume(key=)); ValueError before any launch when
        it is missing, or given for an unkeyed one.  The stream is tagged and released over the
        embedded total (read on the device) and every restored cover's tag is compared, all on
        the device; IntegrityError (.keyed; .slices = covers that failed, .stream = the stream
        failed, whose plaintext then never reaches the host).  verify=False decrypts only."""
        torch = _torch()
        mode = _ck.verify_mode(verify)
        enc = vol.enc
        if enc.scheme != 1 or self.scheme != 1:
            raise ValueError("volume payloads are scheme 1's")
        if (vol.tag is None) != (enc.tag is None):
            raise ValueError("a keyed volume carries both the stream's tag (vol.tag) and the covers' (enc.tag)")
        key = self._keyed_check(enc, key)
        if key is not None:
            _aead._check_tags(vol.tag, 1, self.device, "vol.tag")
        _pv.check_require(mode, key is not None, enc.cover_crc is not None, vol.payload_crc is not None,
                          carrier="the volume")
        self._check_buffers(stego=enc.stego, lm=enc.lm, meta=enc.meta)   # before the records' read-back
        recs = enc.records()
        _raise_lookback(recs)
        _raise_status(recs, "volume, " + self._t_text())
        self._check(enc, recs)
        enc.lengths = [int(r.L) for r in recs]
        sw = max(1, (int(vol.total_bits) + 63) // 64)
        out = torch.empty(sw + 1, dtype=torch.int64, device=self.device)   # the stream, then the total
        cover = torch.empty_like(enc.stego)
        P = self._params(enc.payload_words)
        # the gate is the records': a gated volume decodes on any scheme-1 codec of the shape
        if any(int(r.reserved[1]) != 0 for r in recs):
            fn, what = _lib.load().codec_pee_gvol_extract, "codec_pee_gvol_extract"
            vws = self._gvol_workspace(enc.payload_words, 1)
        else:
            fn, what = _lib.load().codec_pee_volume_extract, "codec_pee_volume_extract"
            vws = self._volume_workspace(enc.payload_words, 1)
        self._guarded(lambda: _lib.check(fn(
            C.byref(P), enc.stego.data_ptr(), enc.meta.data_ptr(), enc.lm.data_ptr(), cover.data_ptr(), out.data_ptr(),
            sw, out.data_ptr() + 8 * sw, self.workspace.data_ptr(), self.workspace.numel(), vws.data_ptr(),
            vws.numel(), _stream()), what))
        host, total = _pv.after_extract(self, enc, cover, out, mode, key, vol=vol)
        return framing.unpack_bits(host, total), cover


def _same_storage(a, b) -> bool:
    return a is b or a.data_ptr() == b.data_ptr()


# one PeeCodec (and its zeroed workspace) per (shape, dtype, T, tmin, tmax, maxval, device); the
# least recently used one is dropped past _CODECS_MAX entries, so varied shapes do not keep
# GPU memory alive indefinitely (clear_codec_cache() drops them all)
_CODECS: "OrderedDict" = OrderedDict()
_CODECS_MAX = 8


def clear_codec_cache():
    """Drop every cached PeeCodec of encode()/decode() (frees their workspaces)."""
    _CODECS.clear()


def _codec_for(shape, dtype: str, *, T, tmax: int, maxval: Optional[int], scheme: int = 1, tmin: int = 1,
               gate=None) -> PeeCodec:
    torch = _torch()
    if maxval is None:
        maxval = 65535 if "16" in dtype else 255
    key = (tuple(shape), dtype, T, int(tmin), int(tmax), int(maxval), int(scheme), torch.cuda.current_device(), gate)
    c = _CODECS.get(key)
    if c is None:
        c = PeeCodec(*shape, dtype=dtype, T=T, tmin=tmin, tmax=tmax, maxval=maxval, scheme=scheme, gate=gate)
        _CODECS[key] = c
        while len(_CODECS) > _CODECS_MAX:
            _CODECS.popitem(last=False)
    else:
        _CODECS.move_to_end(key)
    return c


def _as_gpu_batch(covers):
    """codec._as_batch for encode() / encode_volume(): a numpy array is uploaded; a torch tensor
    must already be on the current GPU, where the cached codec lives (TypeError before any codec
    is built or launch made -- the kernels would take a host pointer as it comes)."""
    from .codec import _as_batch
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(covers, torch.Tensor) and covers.device != dev:
        raise TypeError(f"covers is on {covers.device}, the codec is on {dev}: move the tensor there (numpy arrays "
                        f"are uploaded by the call)")
    return _as_batch(covers)


_STATUS_TEXT = {1: "payload exceeds PEE capacity", _lib.CODEC_PEE_ELOOKBACK: "in-place cursor look-back timed out"}


def _raise_status(recs, what: str):
    """ValueError for capacity overflows (status 1), RuntimeError naming any other code."""
    bad = {}
    for i, r in enumerate(recs):
        if r.status != 0:
            bad.setdefault(int(r.status), []).append(i)
    if not bad:
        return
    if set(bad) == {1}:
        raise ValueError(f"payload exceeds PEE capacity in slices {bad[1]} ({what})")
    text = "; ".join(f"status {c} ({_STATUS_TEXT.get(c, 'unknown status')}) in slices {v}" for c, v in sorted(bad.items()))
    raise RuntimeError(f"codec_pee: {text} ({what})")


def _config_from_records(enc: "PeeEncoded") -> dict:
    """The codec configuration of a PeeEncoded built without one (e.g. by hand): dtype from
    the stego tensor, maxval and T from the per-slice meta records."""
    recs = enc.records()
    if not recs:
        raise ValueError("PeeEncoded holds no slice records")
    dt = "uint16" if _elem_bytes(enc.stego) == 2 else "uint8"
    maxvals = {int(r.maxval) for r in recs}
    if len(maxvals) != 1:
        raise ValueError(f"slices were embedded with different maxval {sorted(maxvals)}; pass a config")
    ts = {int(r.T) for r in recs}
    T = ts.pop() if len(ts) == 1 else "auto"
    tmax = max(16, max(int(r.T) for r in recs))
    cfg = dict(method="pee", T=T, tmax=min(tmax, 64), maxval=maxvals.pop(), dtype=dt)
    gs = {int(r.reserved[1]) - 1 for r in recs if int(r.reserved[1]) != 0}
    if gs:   # informational: decode() takes each slice's gate from its record
        cfg["gate"] = gs.pop() if len(gs) == 1 else "auto"
    return cfg


def encode(covers, payloads: Sequence, *, T=2, tmax: int = 16, maxval: Optional[int] = None,
           scheme: int = 1, tmin: int = 1, checksum=False, gate=None, tile=_TILE_UNSET, roi=None, key=None, nonce=None,
           index0: int = 0) -> PeeEncoded:
    """MED-PEE embed of one payload per slice (the package's `encode(..., method="pee")`).
    covers: [B,H,W] / [H,W] uint8/uint16 torch tensor or numpy array; T: expansion threshold
    or "auto" (smallest T <= tmax whose capacity holds each slice's payload); maxval: the
    largest legal pixel value (e.g. 4095 for 12-bit DICOM; default the dtype's maximum);
    scheme 2: four sublattice passes; its T="auto" tries T = tmin .. tmax per slice in one launch.
    checksum=True: the encoding carries the covers' and payloads' CRC-32 and decode() verifies them.
    checksum="tiles": also one CRC-32 per `tile` (int or (th, tw), 4..1024) of every cover, so that a
    failed verify names the tiles that differ (PeeCodec.embed).
    gate (scheme 1): a smoothness gate 0..65535 or "auto" (PeeCodec); decode() reads it from the records.
    roi (scheme 1): a rectangle (y0, x0, y1, x1) for every slice or [B, 4] of them that the stego leaves
    untouched (PeeCodec.embed); decode() reads it from the records.
    tile: not given = checksum.TILE_DEFAULT (64), as before (PeeCodec.embed explains the marker).
    key / nonce / index0: a keyed embedding (PeeCodec.embed; ChaCha20-Poly1305); decode(enc, key=).
    Raises ValueError when a payload exceeds its slice's capacity."""
    _aead.check_call(key, nonce, fresh=False, lone=None)   # before the GPU is touched
    shape = tuple(covers.shape)
    check_gate_args(gate, T, tmax, (int(shape[-2]) // 2) * (int(shape[-1]) // 2) if len(shape) >= 2 else 0, scheme)
    if roi is not None:   # every rule but the values', which need the batch shape (PeeCodec.embed)
        check_roi_args((0, 0, 0, 0), 1, int(shape[-2]), int(shape[-1]), scheme=scheme, T=T, tmax=tmax, gate=gate,
                       tiled=_ck.checksum_mode(checksum)[1], tile_given=tile is not _TILE_UNSET)
    if _ck.checksum_mode(checksum)[1]:
        _ck.check_tile_args(_ck.TILE_DEFAULT if tile is _TILE_UNSET else tile)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    if isinstance(payloads, (str, bytes, bytearray)):
        payloads = [payloads]
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T=T, tmax=tmax, maxval=maxval, scheme=scheme, tmin=tmin, gate=gate)
    enc = codec.embed(covers, payloads, checksum=checksum, tile=tile, roi=roi, key=key, nonce=nonce, index0=index0)
    if scheme == 2:
        short = [i for i, (g, n) in enumerate(zip(enc.embedded(), enc.lengths)) if g < n]
        if short:
            raise ValueError(f"payload exceeds PEE capacity in slices {short} (scheme 2, {codec._t_text()})")
    else:
        _raise_status(enc.records(), f"T={T}, tmax={tmax}")
    return enc


def decode(enc: PeeEncoded, verify=True, *, restore: bool = True, key=None):
    """Exact extraction: (payload_bit_lists, cover) like the LSB decode() -- payload_bit_lists[b]
    is a numpy 0/1 vector of slice b's embedded bits, cover the restored [B,H,W] tensor
    (None with restore=False).  verify: PeeCodec.decode's (True checks the checksums the
    encoding carries, False skips, 'require' insists on them; IntegrityError on a mismatch).
    key: a keyed embedding's (PeeCodec.decode)."""
    _require_gpu()
    cfg = enc.config or _config_from_records(enc)
    codec = _codec_for(tuple(enc.stego.shape), cfg.get("dtype", "uint16"), T=cfg.get("T", 2),
                       tmax=cfg.get("tmax", 16), maxval=cfg.get("maxval"), scheme=int(getattr(enc, "scheme", 1)),
                       tmin=cfg.get("tmin", 1))
    bits, cover = codec.decode(enc, verify, key=key)
    return bits, (cover if restore else None)


def encode_blind(covers, payloads: Sequence, *, T: int = 2, maxval: Optional[int] = None, checksum=False,
                 max_entries: int = 256, scheme: int = 1, gate=None, roi=None, key=None):
    """Blind MED-PEE embed of one payload per slice (PeeCodec.embed_blind): (stego, info), where the
    stego decodes with nothing beside it (decode_blind).  covers: [B,H,W] / [H,W] uint8 / uint16
    torch tensor or numpy array.  Raises ValueError naming the slices whose payload (with its side
    bits) does not fit; scheme=2, T="auto", gate=, roi= and key= are ValueError before the GPU is
    touched."""
    shape = tuple(covers.shape)
    if len(shape) < 2:
        raise ValueError(f"covers must be [B, H, W] or [H, W], got shape {shape}")
    mv = maxval if maxval is not None else (255 if "8" in str(covers.dtype) and "16" not in str(covers.dtype) else 65535)
    _blind.check_args(scheme=scheme, T=T, gate=gate, H=int(shape[-2]), W=int(shape[-1]), maxval=mv,
                      max_entries=max_entries, roi=roi, key=key)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    if isinstance(payloads, (str, bytes, bytearray)):
        payloads = [payloads]
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T=int(T), tmax=16, maxval=maxval)
    return codec.embed_blind(covers, payloads, checksum=checksum, max_entries=max_entries)


def encode_blind_auto(covers, payloads: Sequence, *, tmax: int = 16, maxval: Optional[int] = None, checksum=False,
                      max_entries: int = 256):
    """encode_blind with T chosen per slice (PeeCodec.embed_blind_auto): (stego, info, ts), each
    slice at the smallest T in 1..tmax that takes its payload.  Raises ValueError naming the slices
    that no T <= tmax serves; argument errors are raised before the GPU is touched."""
    shape = tuple(covers.shape)
    if len(shape) < 2:
        raise ValueError(f"covers must be [B, H, W] or [H, W], got shape {shape}")
    mv = maxval if maxval is not None else (255 if "8" in str(covers.dtype) and "16" not in str(covers.dtype) else 65535)
    _blind.check_args_auto(scheme=1, tmax=tmax, gate=None, H=int(shape[-2]), W=int(shape[-1]), maxval=mv,
                           max_entries=max_entries)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    if isinstance(payloads, (str, bytes, bytearray)):
        payloads = [payloads]
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T=1, tmax=int(tmax), maxval=maxval)
    return codec.embed_blind_auto(covers, payloads, checksum=checksum, max_entries=max_entries)


def encode_blind_gated(covers, payloads: Sequence, *, gate="auto", T=None, tmax: int = 4, maxval: Optional[int] = None,
                       checksum=False, max_entries: int = 256):
    """encode_blind with (T, gate) chosen per slice (PeeCodec.embed_blind_gated): (stego, info, ts, gs);
    decode_blind reads the stego as it is.  Raises ValueError naming the slices that no pair serves;
    argument errors are raised before the GPU is touched."""
    shape = tuple(covers.shape)
    if len(shape) < 2:
        raise ValueError(f"covers must be [B, H, W] or [H, W], got shape {shape}")
    mv = maxval if maxval is not None else (255 if "8" in str(covers.dtype) and "16" not in str(covers.dtype) else 65535)
    _blind.check_args_gated(scheme=1, tmax=tmax, T=T, gate=gate, H=int(shape[-2]), W=int(shape[-1]), maxval=mv,
                            max_entries=max_entries)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    if isinstance(payloads, (str, bytes, bytearray)):
        payloads = [payloads]
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T=1, tmax=16, maxval=maxval)
    return codec.embed_blind_gated(covers, payloads, gate=gate, T=T, tmax=int(tmax), checksum=checksum,
                                   max_entries=max_entries)


def decode_blind(stego, verify=True, *, restore: bool = True):
    """(payload_bit_lists, cover) of a blind stego ([B,H,W] / [H,W] tensor or numpy array), from
    its pixels alone (PeeCodec.decode_blind); cover is None with restore=False."""
    _require_gpu()
    stego = _as_gpu_batch(stego)
    dt = "uint16" if _elem_bytes(stego) == 2 else "uint8"
    codec = _codec_for(tuple(stego.shape), dt, T=2, tmax=16, maxval=None)
    bits, cover = codec.decode_blind(stego, verify=verify)
    return bits, (cover if restore else None)


def encode_blind_volume(covers, payload, *, volume_id=None, policy: str = "even", tmax: int = 16,
                        maxval: Optional[int] = None, checksum=False, max_entries: int = 256):
    """One payload across a [B,H,W] stack of blind stegos (PeeCodec.embed_blind_volume): (stego, info,
    ts).  ValueError when the payload exceeds the stack's capacity at tmax; argument errors are raised
    before the GPU is touched."""
    from . import blind_volume as _bv
    shape = tuple(covers.shape)
    if len(shape) != 3:
        raise ValueError(f"covers must be a [B, H, W] stack, got shape {shape}")
    mv = maxval if maxval is not None else (255 if "8" in str(covers.dtype) and "16" not in str(covers.dtype) else 65535)
    _bv.check_args(scheme=1, tmax=tmax, gate=None, B=int(shape[0]), H=int(shape[1]), W=int(shape[2]), maxval=mv,
                   nbits=int(framing.to_bits(payload).size), policy=policy, max_entries=max_entries, volume_id=volume_id)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T=1, tmax=int(tmax), maxval=maxval)
    return codec.embed_blind_volume(covers, payload, volume_id=volume_id, policy=policy, checksum=checksum,
                                    max_entries=max_entries)


def decode_blind_volume(stego, verify=True, *, partial: bool = False, restore: bool = True):
    """(bits, covers) -- with partial=True (bits, covers, missing) -- of a stack of blind volume
    stegos in any order (PeeCodec.decode_blind_volume); covers is None with restore=False."""
    _require_gpu()
    stego = _as_gpu_batch(stego)
    dt = "uint16" if _elem_bytes(stego) == 2 else "uint8"
    codec = _codec_for(tuple(stego.shape), dt, T=2, tmax=16, maxval=None)
    out = codec.decode_blind_volume(stego, verify=verify, partial=partial)
    return (out[0], out[1] if restore else None) + tuple(out[2:])


def encode_blind_keyed(covers, payloads: Sequence, key, *, T: int = 2, tmax=None, nonce=None, index0: int = 0,
                       maxval: Optional[int] = None, max_entries: int = 256):
    """Keyed blind MED-PEE embed of one payload per slice (PeeCodec.embed_blind_keyed): (stego, info,
    ts), a stego that decode_blind_keyed reads with the key alone.  T: the fixed threshold; tmax in
    1..16: T chosen per slice instead.  Argument errors (key, nonce, index, the blind rules) are
    raised before the GPU is touched."""
    shape = tuple(covers.shape)
    if len(shape) < 2:
        raise ValueError(f"covers must be [B, H, W] or [H, W], got shape {shape}")
    if key is None:
        raise ValueError("encode_blind_keyed takes a 32-byte key; encode_blind is the unkeyed call")
    _aead.check_call(key, nonce, index0, int(shape[0]) if len(shape) > 2 else 1, fresh=False)
    mv = maxval if maxval is not None else (255 if "8" in str(covers.dtype) and "16" not in str(covers.dtype) else 65535)
    if tmax is None:
        _blind.check_args(scheme=1, T=T, gate=None, H=int(shape[-2]), W=int(shape[-1]), maxval=mv, max_entries=max_entries)
    else:
        _blind.check_args_auto(scheme=1, tmax=tmax, gate=None, H=int(shape[-2]), W=int(shape[-1]), maxval=mv,
                               max_entries=max_entries)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    if isinstance(payloads, (str, bytes, bytearray)):
        payloads = [payloads]
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T=int(T) if tmax is None else 1, tmax=16 if tmax is None else int(tmax),
                       maxval=maxval)
    return codec.embed_blind_keyed(covers, payloads, key=key, nonce=nonce, index0=index0, tmax=tmax,
                                   max_entries=max_entries)


def decode_blind_keyed(stego, key, verify=True, *, restore: bool = True):
    """(payload_bit_lists, cover) of a keyed blind stego ([B,H,W] / [H,W] tensor or numpy array) from
    its pixels and the key (PeeCodec.decode_blind_keyed); cover is None with restore=False."""
    _aead.check_key(key)
    _require_gpu()
    stego = _as_gpu_batch(stego)
    dt = "uint16" if _elem_bytes(stego) == 2 else "uint8"
    codec = _codec_for(tuple(stego.shape), dt, T=2, tmax=16, maxval=None)
    bits, cover = codec.decode_blind_keyed(stego, key, verify=verify)
    return bits, (cover if restore else None)


def encode_volume(covers, payload, *, policy: str = "even", tmax: int = 16, maxval: Optional[int] = None,
                  checksum=False, scheme: int = 1, gate=None, tile=_ck.TILE_DEFAULT, key=None, nonce=None,
                  index0: int = 0) -> PeeVolume:
    """MED-PEE embed of ONE payload across a [B,H,W] stack (PeeCodec.embed_volume): the bits are
    spread over the slices on the device (policy "even": in proportion to capacity; "fill": in
    slice order), each slice at the smallest T <= tmax that holds its share.  gate: a smoothness
    gate 0..65535 or "auto" -- a gated volume, planned over (T, G) (PeeCodec.embed_volume);
    decode_volume() reads the gates from the records.  Raises ValueError
    when the volume cannot hold the payload at tmax, as encode() does per slice; argument errors
    (policy, scheme 2, more than 2^31 - 1 bits or candidates, a shape that is no stack) are
    ValueError before the GPU is touched.  key / nonce / index0: a keyed volume (PeeCodec.embed_volume)."""
    _aead.check_call(key, nonce, fresh=False, lone=None)   # before the GPU is touched
    shape = tuple(covers.shape)
    bits = framing.to_bits(payload)
    check_volume_args(shape if len(shape) != 2 else (1,) + shape, bits.size, policy, scheme)
    check_gvol_args(None, gate, tmax, (int(shape[-2]) // 2) * (int(shape[-1]) // 2), scheme)
    if _ck.checksum_mode(checksum)[1]:
        _ck.check_tile_args(tile)
    _require_gpu()
    covers = _as_gpu_batch(covers)
    dt = "uint16" if _elem_bytes(covers) == 2 else "uint8"
    codec = _codec_for(tuple(covers.shape), dt, T="auto", tmax=tmax, maxval=maxval)
    vol = codec.embed_volume(covers, bits, policy=policy, checksum=checksum, gate=gate, tile=tile, key=key, nonce=nonce,
                             index0=index0)
    if vol.embedded_bits < vol.total_bits:
        raise ValueError(f"payload of {vol.total_bits} bits exceeds the volume's PEE capacity "
                         f"{vol.embedded_bits} (tmax={tmax})")
    return vol


def decode_volume(vol: PeeVolume, verify=True, *, restore: bool = True, key=None):
    """(bits, covers) of an encode_volume / embed_volume result: the payload as one 0/1 vector and
    the restored [B,H,W] stack (None with restore=False).  verify: as decode()."""
    _require_gpu()
    enc = vol.enc
    cfg = enc.config or _config_from_records(enc)
    codec = _codec_for(tuple(enc.stego.shape), cfg.get("dtype", "uint16"), T="auto", tmax=cfg.get("tmax", 16),
                       maxval=cfg.get("maxval"))
    bits, cover = codec.decode_volume(vol, verify, key=key)
    return bits, (cover if restore else None)


def _raise_lookback(recs):
    lost = [i for i, r in enumerate(recs) if r.status == _lib.CODEC_PEE_ELOOKBACK]
    if lost:
        raise RuntimeError(f"codec_pee_embed: in-place cursor look-back timed out in slices {lost}; "
                           "their pixels are not a valid stego")


def lm_bits(enc: PeeEncoded, b: int, p: int = 0) -> np.ndarray:
    """Location map of slice b (scheme 2: of pass p) as a bool vector over candidates 0..end."""
    if enc.scheme == 2:
        r = enc.pass_records()[p][b]
        raw = enc.lm[p, b].cpu().numpy().view(np.uint8)
    else:
        r = enc.records()[b]
        raw = enc.lm[b].cpu().numpy().view(np.uint8)
    return np.unpackbits(raw, bitorder="little")[: r.end + 1].astype(bool)

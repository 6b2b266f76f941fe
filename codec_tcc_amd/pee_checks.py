"""The pure-host checks of the MED-PEE layer: record geometry and judgement, the argument rules
of volumes, gates and regions of interest, and the buffer contract of every PeeCodec entry.
ValueError / TypeError before any launch; no GPU and no library load (tests/test_pee_placement.py
holds them to that).  pee.py re-exports every name here."""
from __future__ import annotations

from typing import Optional, Sequence

from . import _lib, roi as _roi
from .codec import _torch


def lattice_geometry(lattice: int, H: int, W: int):
    """(y0, x0, hc, wc) of scheme 2's lattice p: candidate (i, j) is pixel (y0 + 2i, x0 + 2j),
    i < hc, j < wc (include/codec_tcc.h, codec_pee_multi_embed_pass)."""
    ry, rx = ((1, 1), (0, 0), (1, 0), (0, 1))[lattice]
    y0, x0 = (1 if ry else 2), (1 if rx else 2)
    return y0, x0, max(0, (H - y0 + 1) // 2), max(0, (W - x0 + 1) // 2)


def make_record(H: int, W: int, *, T: int, maxval: int, L: int, end: int, status: int, lattice: int = 0,
                gate: Optional[int] = None, roi=None) -> _lib.PeeMeta:
    """The codec_pee_meta an embed of lattice `lattice` writes for this side information (what a
    file header or a side dict of oracle/pee_cpu.py carries); the geometry fields follow from H x W.  The
    values are stored as given -- check_records() judges them.  gate: the smoothness gate G of a
    gated scheme-1 embedding (reserved[1] = G + 1; include/codec_tcc_gate.h), None = ungated.
    roi: the rectangle (y0, x0, y1, x1) of a ROI embedding (reserved[0], reserved[2];
    include/codec_tcc_roi.h); such a record always carries a gate word (65536 without a gate)."""
    _y0, _x0, hc, wc = lattice_geometry(lattice, H, W)
    nc = hc * wc
    m = _lib.PeeMeta()
    m.T, m.maxval, m.L, m.end = int(T), int(maxval), int(L), int(end)
    m.nc, m.ntiles = nc, (nc + 1023) // 1024
    m.tile_end = int(end) // 1024 if int(end) >= 0 else -1
    m.status, m.capacity, m.h, m.w = int(status), int(L), int(H), int(W)
    m.reserved[0] = lattice
    if gate is not None:
        m.reserved[1] = int(gate) + 1
    if roi is not None:
        w0, w2 = _roi.pack_words(roi)
        m.reserved[0], m.reserved[2] = _roi.as_signed(w0), _roi.as_signed(w2)
        if gate is None:
            m.reserved[1] = _lib.GATE_MAX + 1
    return m


def check_records(records, H: int, W: int, *, scheme: int, payload_words: int, lm_words: int, bytes: int,
                  lengths: Optional[Sequence[int]] = None) -> None:
    """Host-side check of MED-PEE side records before a launch that trusts them (a file header,
    hand-made tensors): the extract kernels bound `end`, `L` and the payload row themselves
    (include/codec_tcc.h, record contract) but decode an inconsistent record to garbage, and the
    library cannot look at device-resident records -- so this layer does.  Pure host code: no
    GPU, no library load.

    records: scheme 1 -- one per slice; scheme 2 -- [4][B] pass-major (or the flat 4 * B list of
    PeeEncoded.records()).  lengths (scheme 2): the embedded bits per slice the container
    states, checked against the passes' sum.  Raises ValueError naming slice, pass and field.

    The invariants are those of the records oracle/pee_cpu.py and tests/pee_scalar.py write
    (nc_p = the lattice's candidate count):
      1 <= T <= 64; 1 <= maxval <= the dtype's maximum (the library refuses maxval 0);
      h, w, nc, ntiles = the geometry's; scheme 2: reserved[0] = the pass; scheme 1:
        reserved[1] in 0..65536 (0 = ungated, else the smoothness gate G + 1; a gated record
        obeys every rule below unchanged -- `end` indexes all candidates, active or not);
        scheme 1 with reserved[2] != 0 (a ROI record, include/codec_tcc_roi.h): reserved[0] and
        reserved[2] unpack to y0 < y1 <= H and x0 < x1 <= W, and reserved[1] is in 1..65536;
      status 0: L = 0 and end = -1, or 1 <= L <= end + 1 <= nc_p;
      status 1 (the pass filled up): end = nc_p - 1 and 0 <= L <= nc_p (L = 0 when the
        capacity is 0 and bits were left over);
      status CODEC_PEE_ELOOKBACK (never in files; decode refuses it): only the bounds;
      tile_end = end // 1024 (-1 for end = -1);
      scheme 2: a pass embeds bits only when every earlier pass filled up, and the passes' L
        sum to the stated length;
      64 * payload_words >= the slice's bits; 64 * lm_words > end."""
    if scheme not in (1, 2):
        raise ValueError("scheme must be 1 or 2")
    if bytes not in (1, 2):
        raise ValueError(f"bytes = {bytes}: 1 (uint8) or 2 (uint16)")
    H, W, payload_words, lm_words = int(H), int(W), int(payload_words), int(lm_words)
    if H < 1 or W < 1:
        raise ValueError(f"shape {H} x {W}")
    if payload_words < 1 or lm_words < 1:
        raise ValueError(f"payload_words = {payload_words}, lm_words = {lm_words}: both >= 1")
    npass = 4 if scheme == 2 else 1
    recs = list(records)
    if recs and not isinstance(recs[0], (list, tuple)):
        if len(recs) % npass:
            raise ValueError(f"{len(recs)} records are no multiple of the scheme's {npass} passes")
        n = len(recs) // npass
        recs = [recs[p * n:(p + 1) * n] for p in range(npass)]
    if len(recs) != npass or len({len(pr) for pr in recs}) != 1:
        raise ValueError(f"scheme {scheme} takes {npass} pass(es) of one record per slice")
    B = len(recs[0])
    if lengths is not None and len(lengths) != B:
        raise ValueError(f"{len(lengths)} lengths for {B} slices")
    vmax = 65535 if bytes == 2 else 255

    def bad(b, p, field, value, why):
        raise ValueError(f"MED-PEE record of slice {b}, pass {p}: {field} = {value} ({why})")

    for b in range(B):
        total, filled = 0, True   # filled: every earlier pass has status 1
        for p in range(npass):
            r = recs[p][b]
            _y0, _x0, hc, wc = lattice_geometry(p, H, W)
            nc = hc * wc
            T, maxval, L, end, status = int(r.T), int(r.maxval), int(r.L), int(r.end), int(r.status)
            if not 1 <= T <= 64:
                bad(b, p, "T", T, "1..64")
            if not 1 <= maxval <= vmax:
                bad(b, p, "maxval", maxval, f"1..{vmax}")
            for name, got, want in (("h", r.h, H), ("w", r.w, W), ("nc", r.nc, nc), ("ntiles", r.ntiles, (nc + 1023) // 1024)):
                if int(got) != want:
                    bad(b, p, name, int(got), f"the geometry's is {want}")
            if scheme == 2 and int(r.reserved[0]) != p:
                bad(b, p, "reserved[0]", int(r.reserved[0]), "the pass's lattice")
            if scheme == 1 and not 0 <= int(r.reserved[1]) <= _lib.GATE_MAX + 1:
                bad(b, p, "reserved[1]", int(r.reserved[1]), f"0 (ungated) or a gate + 1 in 1..{_lib.GATE_MAX + 1}")
            if scheme == 1 and int(r.reserved[2]) != 0:   # a ROI record
                y0, x0, y1, x1 = _roi.record_roi(r)
                if not y0 < y1 <= H:
                    bad(b, p, "reserved[2]" if y1 > H else "reserved[0]", int(r.reserved[2] if y1 > H else r.reserved[0]),
                        f"the ROI's rows y0 = {y0}, y1 = {y1}: y0 < y1 <= H = {H}")
                if not x0 < x1 <= W:
                    bad(b, p, "reserved[2]" if x1 > W else "reserved[0]", int(r.reserved[2] if x1 > W else r.reserved[0]),
                        f"the ROI's columns x0 = {x0}, x1 = {x1}: x0 < x1 <= W = {W}")
                if int(r.reserved[1]) == 0:
                    bad(b, p, "reserved[1]", 0, f"a ROI record carries a gate + 1 in 1..{_lib.GATE_MAX + 1}")
            if status == 0:
                if L == 0:
                    if end != -1:
                        bad(b, p, "end", end, "-1 when no bit is embedded")
                elif L < 0:
                    bad(b, p, "L", L, ">= 0")
                elif not 0 <= end < nc:
                    bad(b, p, "end", end, f"0..{nc - 1}, the lattice's candidates")
                elif L > end + 1:
                    bad(b, p, "L", L, f"at most end + 1 = {end + 1}")
            elif status == 1:
                if end != nc - 1:
                    bad(b, p, "end", end, f"{nc - 1}: a pass that filled up processes every candidate")
                if not 0 <= L <= nc:
                    bad(b, p, "L", L, f"0..{nc}")
            elif status == _lib.CODEC_PEE_ELOOKBACK:
                if not -1 <= end < nc:
                    bad(b, p, "end", end, f"-1..{nc - 1}")
                if L < 0:
                    bad(b, p, "L", L, ">= 0")
            else:
                bad(b, p, "status", status, f"0, 1 or {_lib.CODEC_PEE_ELOOKBACK}")
            if int(r.tile_end) != (end // 1024 if end >= 0 else -1):
                bad(b, p, "tile_end", int(r.tile_end), f"end // 1024 = {end // 1024 if end >= 0 else -1}")
            if end >= 64 * lm_words:
                bad(b, p, "end", end, f"past the location map's {64 * lm_words} bits")
            if L > 0 and not filled:
                bad(b, p, "L", L, "bits embedded after a pass that did not fill up")
            filled = filled and status == 1
            total += L
        if total > 64 * payload_words:
            bad(b, npass - 1, "L", total, f"the slice's bits exceed the payload row's {64 * payload_words}")
        if scheme == 2 and lengths is not None and int(lengths[b]) != total:
            bad(b, npass - 1, "L", total, f"the passes' sum; the stated length is {int(lengths[b])}")


VOLUME_NMAX = 2 ** 31 - 1   # include/codec_tcc_vol.h: bits of one volume stream, and B * (H//2) * (W//2)


def check_volume_args(shape, nbits: int, policy: str = "even", scheme: int = 1) -> None:
    """The argument rules of a volume embed (include/codec_tcc_vol.h), as ValueError before any
    launch.  Pure host code: no GPU, no library load."""
    if int(scheme) != 1:
        raise ValueError("volume payloads are scheme 1's: scheme 2 has no cover-side capacity to plan with "
                         "(DESIGN §3b-2)")
    if policy not in _lib.VOL_POLICIES:
        raise ValueError(f"policy must be one of {sorted(_lib.VOL_POLICIES)}, got {policy!r}")
    if len(shape) != 3 or min(int(v) for v in shape) < 1:
        raise ValueError(f"a volume is a [B, H, W] stack with no empty dimension, got shape {tuple(shape)}")
    B, H, W = (int(v) for v in shape)
    if B * (H // 2) * (W // 2) > VOLUME_NMAX:
        raise ValueError(f"B * (H // 2) * (W // 2) = {B * (H // 2) * (W // 2)} candidates exceed 2^31 - 1")
    if not 0 <= int(nbits) <= VOLUME_NMAX:
        raise ValueError(f"a volume payload holds 0 .. 2^31 - 1 bits, got {int(nbits)}")


def check_gate_args(gate, T, tmax: int, nc: int, scheme: int = 1) -> None:
    """The argument rules of a smoothness gate (include/codec_tcc_gate.h), as ValueError before
    any launch.  Pure host code: no GPU, no library load.  gate: None, 0..65535 or "auto"."""
    if gate is None:
        return
    if int(scheme) != 1:
        raise ValueError("the smoothness gate is scheme 1's: scheme 2's neighbours are modified by its earlier "
                         "passes (DESIGN §3f)")
    if isinstance(gate, str):
        if gate != "auto":
            raise ValueError("gate must be None, an integer in 0..65535 or 'auto'")
    elif isinstance(gate, bool) or int(gate) != gate or not 0 <= int(gate) <= _lib.GATE_MAX:
        raise ValueError(f"gate must be None, an integer in 0..{_lib.GATE_MAX} or 'auto', got {gate!r}")
    if not 1 <= int(tmax) <= _lib.GATE_TMAX:
        raise ValueError(f"a gated codec takes tmax in 1..{_lib.GATE_TMAX} (the selection's 64-bit products), got {tmax}")
    if gate == "auto" and not isinstance(T, str) and not 1 <= int(T) <= int(tmax):
        raise ValueError(f"gate='auto' with a fixed T takes T in 1..tmax = {int(tmax)}, got {T}")
    if int(nc) > _lib.GATE_MAX_NC:
        raise ValueError(f"{int(nc)} candidates per slice exceed the gated selection's 2^26")


def check_roi_args(roi, B: int, H: int, W: int, *, scheme: int = 1, T=None, tmax: int = 16, gate=None, tiled: bool = False,
                   tile_given: bool = True):
    """The argument rules of embed(..., roi=) (include/codec_tcc_roi.h), as ValueError before
    anything is queued; returns roi.normalize_roi's host array (None for roi=None).  Pure host
    code but for the read-back of a device tensor's values."""
    if roi is None:
        return None
    if int(scheme) != 1:
        raise ValueError("a region of interest is scheme 1's: scheme 2's later passes modify the pixels scheme 1 "
                         "leaves alone (DESIGN §3i)")
    if tiled and not tile_given:
        raise ValueError("roi= with checksum='tiles' takes an explicit tile=: choose the grid with the rectangle in "
                         "view (DESIGN §3i)")
    _roi.check_roi_shape(H, W)
    nc = (int(H) // 2) * (int(W) // 2)
    if gate is None:   # the ROI calls are gated calls: the table and the selection's limits apply
        if T == "auto" and not 1 <= int(tmax) <= _lib.GATE_TMAX:
            raise ValueError(f"roi= with T='auto' takes tmax in 1..{_lib.GATE_TMAX} (the gated selection's), got {tmax}")
        if nc > _lib.GATE_MAX_NC:
            raise ValueError(f"{nc} candidates per slice exceed the gated selection's 2^26")
    return _roi.normalize_roi(roi, B, H, W)


def check_gvol_args(codec_gate, gate, tmax: int, nc: int, scheme: int = 1) -> None:
    """The argument rules of embed_volume's gate= keyword (include/codec_tcc_gvol.h), as
    ValueError before any launch.  Pure host code: no GPU, no library load.  codec_gate: the
    gate the codec itself was built with (must be None: a volume takes its gate per call)."""
    if codec_gate is not None:
        raise ValueError("volume payloads take an ungated codec: a codec built with gate= plans per slice "
                         "(DESIGN §3f); build the codec without gate= and pass embed_volume(..., gate=) to plan "
                         "a gated volume over (T, G) (DESIGN §3g)")
    if gate is not None and int(scheme) != 1:
        raise ValueError("volume payloads are scheme 1's: scheme 2 has no cover-side capacity to plan with "
                         "(DESIGN §3b-2)")
    check_gate_args(gate, "auto", tmax, nc, scheme)


def _check_multi_args(B: int, lm_words: int, meta, lm, *, payload=None, payload_words: Optional[int] = None):
    """Scheme 2's argument shapes (the library reads 4 * B records and maps, and with `payload`
    writes B rows of payload_words words): ValueError before any launch.  Shapes only -- runs
    on tensors of any device."""
    if tuple(lm.shape) != (4, B, lm_words) or tuple(meta.shape) != (4, B, _lib.PEE_META_BYTES):
        raise ValueError("scheme 2 takes lm [4, B, lm_words] and meta [4, B, PEE_META_BYTES]")
    if lm.element_size() != 8 or meta.element_size() != 1:
        raise ValueError("scheme 2 takes lm as 64-bit words and meta as bytes")
    if not (lm.is_contiguous() and meta.is_contiguous()):
        raise ValueError("scheme 2's lm and meta must be contiguous")
    if payload is not None:
        pw = int(payload_words)
        if pw < 1 or payload.dim() != 2 or payload.shape[0] != B or payload.shape[1] < pw or payload.element_size() != 8:
            raise ValueError(f"the payload buffer must hold at least [B, payload_words] = [{B}, {pw}] 64-bit words")
        if payload.stride(1) != 1 or (B > 1 and payload.stride(0) != pw):
            raise ValueError("the payload buffer's rows must be payload_words words apart (the library's row pitch)")


_PIX_DTYPES = {}
_INT32 = []


def _pix_dtypes(nbytes: int):
    if not _PIX_DTYPES:
        torch = _torch()
        _INT32.append(torch.int32)
        _PIX_DTYPES.update({1: (torch.uint8,), 2: (torch.uint16, torch.int16)})
    return _PIX_DTYPES[nbytes]


def _on_device(t, device) -> bool:
    """t is a torch tensor on `device` (a device given without an index names every card of its type)."""
    if not isinstance(t, _torch().Tensor):
        return False
    d = t.device
    return d == device or (device.index is None and d.type == device.type)


def _dense(t, device, shape, esize: int) -> bool:
    return _on_device(t, device) and t.shape == shape and t.element_size() == esize and t.is_contiguous()


def _bad_device(name: str, t, device):
    if not isinstance(t, _torch().Tensor):
        raise TypeError(f"{name} must be a torch tensor on {device}, got {type(t).__name__}")
    raise TypeError(f"{name} is on {t.device}, the codec is on {device}")


# What check_buffers calls once an argument failed its one-expression test: the rules again, one by
# one, with the message.  They return when nothing is wrong after all -- the quick test compares
# devices exactly, and a codec device given without an index names every card of its type.
def _bad_pixels(name: str, t, device, shape, nbytes: int):
    if not _on_device(t, device):
        _bad_device(name, t, device)
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have the codec's shape {shape}, got {tuple(t.shape)}")
    if t.dtype not in _pix_dtypes(nbytes):
        raise ValueError(f"{name} must hold {nbytes}-byte pixels (uint{8 * nbytes}), got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (a dense [B, H, W] block at any storage offset), got strides "
                         f"{tuple(t.stride())}: the library sees a pointer and (B, H, W) alone")


def _bad_side(name: str, t, device, rest, what: str):
    """rest(): every rule of the argument but the device's."""
    if not _on_device(t, device):
        _bad_device(name, t, device)
    if not rest():
        raise ValueError(f"{name} must be {what}, got shape {tuple(t.shape)}, strides {tuple(t.stride())}, {t.dtype}")


def _bad_overlap(src_name: str, dst_name: str, apart: int, nbytes: int):
    raise ValueError(f"{dst_name} overlaps {src_name} without being the same buffer ({apart} bytes apart, {nbytes} "
                     f"bytes each): pass the same tensor (in place) or disjoint buffers")


def check_buffers(device, B: int, H: int, W: int, bytes: int, *, lm_words: Optional[int] = None, scheme: int = 1,
                  covers=None, stego=None, cover=None, lm=None, meta=None, payload=None,
                  payload_words: Optional[int] = None, packed=None) -> None:
    """The buffer contract of every PeeCodec entry that hands a pointer to the library, which
    sees that pointer and (B, H, W, bytes) alone and assumes a dense block on the current
    device: TypeError / ValueError naming the argument, before anything is queued.  Shapes,
    strides, devices and pointers only -- it runs on tensors of any device without a GPU, and
    makes no launch, sync, allocation or read-back.  Arguments left None are not looked at.

    covers, stego, cover (the pixel tensors): torch tensors on `device` (TypeError naming both
      devices otherwise), of shape (B, H, W), `bytes`-byte pixels, contiguous -- at any storage
      offset: big[lo:hi] or flat[k:k + n].view(B, H, W) are dense blocks; a crop, a strided or
      a transposed view is not;
    the call's source and destination (covers -> stego, stego -> cover) are the same pointer
      (in place) or disjoint byte ranges: the out-of-place kernels look back at neighbours
      through __restrict__ pointers;
    lm: [B, lm_words] 64-bit words, contiguous; meta: [B, PEE_META_BYTES] bytes, contiguous
      (scheme 2: [4, B, ...] each, as _check_multi_args has them);
    payload: at least [B, payload_words] 64-bit words whose rows are payload_words apart;
    packed = (words, lengths, lens_t): words [B, pw >= 1] 64-bit, contiguous; one length per
      slice; lens_t int32 [B], contiguous.

    This runs on every embed and extract, launch-bound ones included: each argument is one
    expression of attribute reads, and nothing else happens (no call, no string) unless it fails."""
    try:
        shape = (B, H, W)
        dts = _PIX_DTYPES[bytes] if _PIX_DTYPES else _pix_dtypes(bytes)
        if covers is not None and not (covers.device == device and covers.shape == shape and covers.dtype in dts
                                       and covers.is_contiguous()):
            _bad_pixels("covers", covers, device, shape, bytes)
        if stego is not None:
            if not (stego.device == device and stego.shape == shape and stego.dtype in dts and stego.is_contiguous()):
                _bad_pixels("stego", stego, device, shape, bytes)
            if covers is not None and covers is not stego:
                apart = covers.data_ptr() - stego.data_ptr()
                if apart and -B * H * W * bytes < apart < B * H * W * bytes:
                    _bad_overlap("covers", "stego", abs(apart), B * H * W * bytes)
        if cover is not None:
            if not (cover.device == device and cover.shape == shape and cover.dtype in dts and cover.is_contiguous()):
                _bad_pixels("cover", cover, device, shape, bytes)
            if stego is not None and stego is not cover:
                apart = stego.data_ptr() - cover.data_ptr()
                if apart and -B * H * W * bytes < apart < B * H * W * bytes:
                    _bad_overlap("stego", "cover", abs(apart), B * H * W * bytes)
        if lm is not None:   # scheme 2: one map and one record per pass, pass-major
            want = (4, B, lm_words) if scheme == 2 else (B, lm_words)
            if not (lm.device == device and lm.shape == want and lm.element_size() == 8 and lm.is_contiguous()):
                _bad_side("lm", lm, device, lambda: _dense(lm, lm.device, want, 8),
                          f"{list(want)} ([B, lm_words]; scheme 2: [4, B, lm_words]) contiguous 64-bit words")
        if meta is not None:
            want = (4, B, _lib.PEE_META_BYTES) if scheme == 2 else (B, _lib.PEE_META_BYTES)
            if not (meta.device == device and meta.shape == want and meta.element_size() == 1 and meta.is_contiguous()):
                _bad_side("meta", meta, device, lambda: _dense(meta, meta.device, want, 1),
                          f"{list(want)} ([B, PEE_META_BYTES]; scheme 2: [4, B, PEE_META_BYTES]) contiguous bytes")
        if payload is not None:
            pw = int(payload_words)
            sh = payload.shape
            if not (payload.device == device and pw >= 1 and len(sh) == 2 and sh[0] == B and sh[1] >= pw
                    and payload.element_size() == 8 and payload.stride() == (pw, 1)):   # B = 1: any row pitch, below
                _bad_side("payload", payload, device, lambda: pw >= 1 and len(sh) == 2 and sh[0] == B and sh[1] >= pw
                          and payload.element_size() == 8, f"at least [B, payload_words] = [{B}, {pw}] 64-bit words")
                _bad_side("payload", payload, device, lambda: payload.stride(1) == 1 and (B == 1 or payload.stride(0) == pw),
                          f"rows of 64-bit words payload_words = {pw} apart (the library's row pitch)")
        if packed is not None:
            words, lengths, lens_t = packed
            sh = words.shape
            if not (words.device == device and len(sh) == 2 and sh[0] == B and sh[1] >= 1 and words.element_size() == 8
                    and words.is_contiguous()):
                _bad_side("packed[0]", words, device, lambda: len(sh) == 2 and sh[0] == B and sh[1] >= 1
                          and words.element_size() == 8 and words.is_contiguous(),
                          f"[B, payload_words >= 1] = [{B}, >= 1] contiguous 64-bit words")
            if len(lengths) != B:
                raise ValueError(f"packed[1] holds {len(lengths)} lengths for {B} slices")
            if not (lens_t.device == device and lens_t.shape == (B,) and lens_t.dtype == _INT32[0]
                    and lens_t.is_contiguous()):
                _bad_side("packed[2]", lens_t, device, lambda: _dense(lens_t, lens_t.device, (B,), 4)
                          and lens_t.dtype == _torch().int32, f"[B] = [{B}] contiguous int32 lengths")
    except AttributeError:   # something that is no tensor at all
        named = (("covers", covers), ("stego", stego), ("cover", cover), ("lm", lm), ("meta", meta), ("payload", payload))
        named += (("packed[0]", packed[0]), ("packed[2]", packed[2])) if packed is not None and len(packed) == 3 else ()
        for name, t in named:
            if t is not None and not isinstance(t, _torch().Tensor):
                _bad_device(name, t, device)
        raise

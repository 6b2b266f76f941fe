"""The ".bin" container ("STGC") either side of the pixel path.

Version 1 is byte-compatible with the reference (codec.py:601-750):

    b"STGC" | >I header_length | header | zlib(dense bitmaps) | compressed stego
    header v1 = >BBBBHHH (version=1, codec_id, s, align, width, height, start_offset)
                + s*>H segments_lengths + s*>B segment_indices + >I bitmaps_blob_size

Its 16-bit fields overflow at 2048^2 (struct.error) and main() writes
start_offset=0 (codec.py:903).  Version 2 (this build's extension) widens width, height,
start_offset and segments_lengths to 32 bits (segments_lengths signed: T < s plans have
negative sizes) and stores the real offset:

    header v2 = >BBBBIIi (version=2, codec_id, s, align, width, height, start_offset)
                + s*>i segments_lengths + s*>B segment_indices + >I bitmaps_blob_size
                [+ >H search_block_size]   (optional; 0 / absent = unknown)

MED-PEE files (this build's scheme; the reference has no PEE format) use
the same magic and framing with version 16:

    header pee = >BBBB (version=16, codec_id, bytes per pixel, scheme byte 0)
                 + >II (width, height) + >iiiii (T, L = embedded bits, end, maxval, status)
                 + >I lm_blob_size
    body       = zlib(location-map bits of candidates 0..end, LSB-first) | compressed stego

MED-PEE scheme 2 (four sublattice passes, oracle/pee_cpu.py) sets the scheme byte to 2:

    header pee2 = >BBBB (version=16, codec_id, bytes per pixel, 2)
                  + >II (width, height) + >iiii (T, maxval, L = embedded bits, status)
                  + 4 x >iiiI (L_p, end_p, status_p, lm_blob_size_p)
    body        = the 4 passes' zlib location maps in pass order | compressed stego

so a reader of scheme-1 files (scheme byte 0) refuses scheme-2 files instead of misreading.

Either MED-PEE header may end with the 10-byte checksum extension b"C1" + >II (CRC-32 of the
cover, CRC-32 of the embedded payload bits; checksum.py), and that may be followed by the tile
extension b"T1" + >HHHH (th, tw, nty, ntx) + nty * ntx x >I (the cover's CRC-32 per tile).  Readers slice the fixed fields by
size, so files with it read where it is unknown and files without it are unchanged.

Stego payload codecs: the reference's ids (png 1, j2k 2, jls 3, jxl 4) are kept; id 0
("raw", unknown to the reference) stores the stego pixels little-endian, uncompressed.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAGIC = b"STGC"
PEE_VERSION = 16
CODEC_IDS = {"png": 1, "j2k": 2, "jls": 3, "jxl": 4}     # codec.py:616
CODEC_NAMES = {1: "png", 2: "j2k", 3: "jls", 4: "jxl"}   # codec.py:693


def create_header(codec: str, s: int, segments_lengths: Sequence[int], segments_indices: Sequence[int],
                  bitmaps_blob_size: int, width: int, height: int, start_offset: int,
                  align_across_planes: bool, version: int = 1, search_block_size: Optional[int] = None) -> bytes:
    """codec.py:601-656 (version 1, identical bytes; raises struct.error where it does).
    Version 2 may also record the block size of the start-offset search."""
    cid = CODEC_IDS.get(codec.lower(), 0)
    flag = 1 if align_across_planes else 0
    if version == 1:
        fmt = ">BBBBHHH" + f"{s}H" + f"{s}B" + "I"
    elif version == 2:
        fmt = ">BBBBIIi" + f"{s}i" + f"{s}B" + "I"
    else:
        raise ValueError(f"unknown container version {version}")
    hdr = struct.pack(fmt, version, cid, s, flag, width, height, start_offset,
                      *list(segments_lengths), *list(segments_indices), bitmaps_blob_size)
    if version == 2 and search_block_size is not None:
        hdr += struct.pack(">H", int(search_block_size))
    return hdr


def create_binary_file(filename: str, header_bytes: bytes, stego_compressed: bytes, bitmaps_bytes: bytes) -> int:
    """codec.py:658-670: STGC + >I len + header + bitmap blob + stego; returns the file size."""
    with open(filename, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack(">I", len(header_bytes)))
        f.write(header_bytes)
        f.write(bitmaps_bytes)
        f.write(stego_compressed)
    return os.path.getsize(filename)


def parse_bin_bytes(data: bytes) -> Tuple[Dict, bytes, bytes]:
    if data[:4] != MAGIC:
        raise ValueError("Arquivo inválido ou com assinatura incorreta.")   # codec.py:698
    # a foreign file is refused here, as ValueError, before its fields reach a kernel: a cut
    # header, a plane count the records cannot hold, an empty image, a blob past the body
    if len(data) < 8:
        raise ValueError("truncated STGC file: no header length")
    (hlen,) = struct.unpack(">I", data[4:8])
    hdr = data[8:8 + hlen]
    if len(hdr) < hlen:
        raise ValueError(f"truncated STGC file: the header needs {hlen} bytes, the file holds {len(hdr)}")
    if hlen < 1:
        raise ValueError("truncated STGC header: no version byte")
    version = hdr[0]
    if version == PEE_VERSION:
        raise ValueError("a MED-PEE container (version 16): use parse_pee_bytes / decode_bin_pee")
    if version not in (1, 2):
        raise ValueError(f"unknown STGC container version {version}")
    base = ">BBBBHHH" if version == 1 else ">BBBBIIi"
    nb = struct.calcsize(base)
    if hlen < nb:
        raise ValueError(f"truncated STGC header: {hlen} bytes, the fixed fields need {nb}")
    version, cid, s, flag, width, height, start = struct.unpack(base, hdr[:nb])
    if not 1 <= s <= 16:
        raise ValueError(f"STGC header: s = {s} local planes (1..16)")
    if width * height == 0:
        raise ValueError(f"STGC header: width x height = {width} x {height}")
    lf = f">{s}H" if version == 1 else f">{s}i"
    nl = struct.calcsize(lf)
    if hlen < nb + nl + s + 4:
        raise ValueError(f"truncated STGC header: {hlen} bytes, s = {s} needs {nb + nl + s + 4}")
    lens = list(struct.unpack(lf, hdr[nb:nb + nl]))
    idx = list(struct.unpack(f">{s}B", hdr[nb + nl:nb + nl + s]))
    (blob_size,) = struct.unpack(">I", hdr[nb + nl + s:nb + nl + s + 4])
    rest = hdr[nb + nl + s + 4:]
    body = data[8 + hlen:]
    if blob_size > len(body):
        raise ValueError(f"truncated STGC file: a bitmap blob of {blob_size} bytes, {len(body)} left")
    md = {"version": version, "codec": CODEC_NAMES.get(cid, "unknown"), "s": s, "align_flag": flag,
          "width": width, "height": height, "start_offset": start, "segments_lengths": lens,
          "segments_indices": idx}
    if version == 2 and len(rest) >= 2:
        md["search_block_size"] = struct.unpack(">H", rest[:2])[0] or None
    return md, body[:blob_size], body[blob_size:]


def parse_bin_file(filepath: str) -> Tuple[Dict, bytes, bytes]:
    """codec.py:689-750 -> (metadata, bitmaps_blob, stego_bytes)."""
    with open(filepath, "rb") as f:
        return parse_bin_bytes(f.read())


def bitmaps_blob(dense: np.ndarray) -> bytes:
    """zlib of the stacked s x H x W uint8 bitmaps (codec.py:888-889)."""
    return zlib.compress(np.ascontiguousarray(dense, dtype=np.uint8).tobytes())


def split_bitmaps(blob: bytes, s: int) -> List[np.ndarray]:
    """codec.py:820-821: zlib.decompress + np.split into s flat planes."""
    return np.split(np.frombuffer(zlib.decompress(blob), dtype=np.uint8), s)


def encode_stego_raw(stego: np.ndarray) -> bytes:
    return np.ascontiguousarray(stego).astype(stego.dtype.newbyteorder("<"), copy=False).tobytes()


def decode_stego_raw(data: bytes, height: int, width: int) -> np.ndarray:
    npx = height * width
    itemsize = len(data) // npx if npx else 0
    if itemsize not in (1, 2) or itemsize * npx != len(data):
        raise ValueError("raw stego payload does not match the header's width x height")
    return np.frombuffer(data, dtype="<u2" if itemsize == 2 else np.uint8).reshape(height, width).astype(
        np.uint16 if itemsize == 2 else np.uint8)


# ------------------------------------------------------------------ MED-PEE container
_PEE_FMT = ">BBBBIIiiiiiI"


def create_pee_header(codec: str, bytes_per_px: int, width: int, height: int, T: int, L: int, end: int,
                      maxval: int, status: int, lm_blob_size: int) -> bytes:
    return struct.pack(_PEE_FMT, PEE_VERSION, CODEC_IDS.get(codec.lower(), 0), int(bytes_per_px), 0, width, height,
                       int(T), int(L), int(end), int(maxval), int(status), int(lm_blob_size))


def lm_blob(lm_bits: np.ndarray) -> bytes:
    """zlib of the location-map bits (candidates 0..end), packed LSB-first."""
    return zlib.compress(np.packbits(np.asarray(lm_bits, dtype=np.uint8), bitorder="little").tobytes())


def lm_from_blob(blob: bytes, end: int) -> np.ndarray:
    """Location-map bits of candidates 0..end.  ValueError for a blob that is not zlib or
    holds fewer than end + 1 bits; at most the bytes those bits need are inflated (one more,
    to see that nothing follows), so a tiny blob cannot inflate without bound."""
    end = int(end)
    if end < 0:
        return np.zeros(0, dtype=bool)
    need = (end + 8) // 8
    d = zlib.decompressobj()
    try:
        out = d.decompress(bytes(blob), need + 1)
    except zlib.error as exc:
        raise ValueError(f"MED-PEE location-map blob is not valid zlib data ({exc})") from None
    if len(out) > need:
        raise ValueError(f"MED-PEE location-map blob inflates past the {need} bytes of end + 1 = {end + 1} bits")
    if not d.eof:   # every input byte was consumed (the output limit was not reached)
        raise ValueError("MED-PEE location-map blob is a truncated zlib stream")
    if len(out) < need:
        raise ValueError(f"MED-PEE location-map blob holds {8 * len(out)} bits, fewer than end + 1 = {end + 1}")
    return np.unpackbits(np.frombuffer(out, dtype=np.uint8), bitorder="little")[: end + 1].astype(bool)


def _pee_header(data: bytes, fmt_bytes: int, what: str) -> Tuple[bytes, bytes]:
    """(header, body) of a version-16 file whose header holds at least fmt_bytes bytes
    (structure only: the field values are checked where the records are built)."""
    (hlen,) = struct.unpack(">I", data[4:8])   # pee_scheme() saw the magic and 4 header bytes
    hdr = data[8:8 + hlen]
    if len(hdr) < hlen:
        raise ValueError(f"truncated {what}: the header needs {hlen} bytes, the file holds {len(hdr)}")
    if hlen < fmt_bytes:
        raise ValueError(f"truncated {what}: a header of {hlen} bytes, {fmt_bytes} needed")
    return hdr, data[8 + hlen:]


_PEE_CRC_TAG = b"C1"
_PEE_CRC_FMT = ">II"


def pee_crc_extension(cover_crc32: int, payload_crc32: int) -> bytes:
    """The 10-byte header extension of a checksummed MED-PEE file: b"C1" + the cover's and the
    payload's CRC-32 (checksum.py), appended after the header's fixed fields.  Readers slice the
    header by its fixed size, so files with it read as before where it is not known."""
    return _PEE_CRC_TAG + struct.pack(_PEE_CRC_FMT, int(cover_crc32) & 0xFFFFFFFF, int(payload_crc32) & 0xFFFFFFFF)


def _pee_crc_fields(ext: bytes) -> Dict:
    """{'cover_crc32', 'payload_crc32'} of the header bytes after the fixed fields ({} when they
    do not start the checksum extension); ValueError for a header cut inside it."""
    n = len(_PEE_CRC_TAG) + struct.calcsize(_PEE_CRC_FMT)
    if not ext or ext[:2] != _PEE_CRC_TAG[:len(ext[:2])]:
        return {}
    if len(ext) < n:
        raise ValueError(f"truncated MED-PEE header: a checksum extension of {len(ext)} bytes, {n} needed")
    c, p = struct.unpack(_PEE_CRC_FMT, ext[2:n])
    return {"cover_crc32": c, "payload_crc32": p}


_PEE_TILE_TAG = b"T1"
_PEE_TILE_FMT = ">HHHH"
_TILE_MIN, _TILE_MAX = 4, 1024   # include/codec_tcc_tile.h


def pee_tile_extension(th: int, tw: int, table) -> bytes:
    """The second header extension of a MED-PEE file written with checksum="tiles", appended after
    the 10-byte b"C1" extension: b"T1" + >HHHH (th, tw, nty, ntx) + nty * ntx x >I, the cover's
    tile checksums row-major (checksum.tiles_host's table [nty, ntx]).  Readers that know only
    b"C1" ignore what follows it, so they still read the file and verify the slice CRC."""
    t = np.asarray(table)
    if t.ndim != 2 or t.size == 0:
        raise ValueError("a tile table is a non-empty [nty, ntx] array")
    nty, ntx = t.shape
    if not (_TILE_MIN <= int(th) <= _TILE_MAX and _TILE_MIN <= int(tw) <= _TILE_MAX):
        raise ValueError(f"tile size ({th}, {tw}) outside {_TILE_MIN}..{_TILE_MAX}")
    if nty > 0xFFFF or ntx > 0xFFFF:
        raise ValueError(f"a tile grid of {nty} x {ntx} does not fit the extension's 16-bit fields")
    words = (t.astype(np.int64) & 0xFFFFFFFF).astype(">u4")
    return _PEE_TILE_TAG + struct.pack(_PEE_TILE_FMT, int(th), int(tw), nty, ntx) + words.tobytes()


def _pee_tile_fields(ext: bytes, width: int, height: int) -> Dict:
    """{'tile': (th, tw), 'tile_crc32': uint32 [nty, ntx]} of the header bytes after the b"C1"
    extension ({} when they do not start the tile extension); ValueError for a header cut inside
    it, a tile size out of range or a grid that is not ceil(height / th) x ceil(width / tw)."""
    if not ext or ext[:2] != _PEE_TILE_TAG[:len(ext[:2])]:
        return {}
    n0 = len(_PEE_TILE_TAG) + struct.calcsize(_PEE_TILE_FMT)
    if len(ext) < n0:
        raise ValueError(f"truncated MED-PEE header: a tile extension of {len(ext)} bytes, at least {n0} needed")
    th, tw, nty, ntx = struct.unpack(_PEE_TILE_FMT, ext[2:n0])
    if not (_TILE_MIN <= th <= _TILE_MAX and _TILE_MIN <= tw <= _TILE_MAX):
        raise ValueError(f"MED-PEE header: tile size ({th}, {tw}) outside {_TILE_MIN}..{_TILE_MAX}")
    if (nty, ntx) != (-(-height // th), -(-width // tw)):
        raise ValueError(f"MED-PEE header: a tile grid of {nty} x {ntx} contradicts {height} x {width} pixels at "
                         f"tile ({th}, {tw})")
    n = n0 + 4 * nty * ntx
    if len(ext) < n:
        raise ValueError(f"truncated MED-PEE header: a tile extension of {len(ext)} bytes, {n} needed")
    table = np.frombuffer(ext[n0:n], dtype=">u4").astype(np.uint32).reshape(nty, ntx)
    return {"tile": (th, tw), "tile_crc32": table}


_PEE_AEAD_TAG = b"A1"
_PEE_AEAD_NONCE, _PEE_AEAD_MAC = 8, 16


def pee_aead_extension(nonce: bytes, tag: bytes) -> bytes:
    """The header extension of a keyed MED-PEE file: b"A1" + the 8-byte nonce + the
    16-byte Poly1305 tag, appended after whichever of the b"C1" / b"T1" extensions are present, or
    directly after the fixed fields.  Readers that do not know it ignore it (and read ciphertext)."""
    if not isinstance(nonce, (bytes, bytearray)) or len(nonce) != _PEE_AEAD_NONCE:
        raise ValueError(f"the nonce of the keyed extension has {_PEE_AEAD_NONCE} bytes")
    if not isinstance(tag, (bytes, bytearray)) or len(tag) != _PEE_AEAD_MAC:
        raise ValueError(f"the tag of the keyed extension has {_PEE_AEAD_MAC} bytes")
    return _PEE_AEAD_TAG + bytes(nonce) + bytes(tag)


def _pee_aead_fields(ext: bytes) -> Dict:
    """{'aead_nonce', 'aead_tag'} of the header bytes after the other extensions ({} when they do
    not start the keyed extension); ValueError for a header cut inside it."""
    if not ext or ext[:2] != _PEE_AEAD_TAG[:len(ext[:2])]:
        return {}
    n = len(_PEE_AEAD_TAG) + _PEE_AEAD_NONCE + _PEE_AEAD_MAC
    if len(ext) < n:
        raise ValueError(f"truncated MED-PEE header: a keyed extension of {len(ext)} bytes, {n} needed")
    return {"aead_nonce": bytes(ext[2:2 + _PEE_AEAD_NONCE]), "aead_tag": bytes(ext[2 + _PEE_AEAD_NONCE:n])}


def _pee_ext_fields(ext: bytes, width: int, height: int) -> Dict:
    """The fields of a header's extensions: the checksum extension's, the tile extension's when
    it follows, and the keyed extension's after whichever of them are present."""
    md = _pee_crc_fields(ext)
    rest = ext
    if md:
        rest = ext[len(_PEE_CRC_TAG) + struct.calcsize(_PEE_CRC_FMT):]
        tiles = _pee_tile_fields(rest, width, height)
        if tiles:
            md.update(tiles)
            rest = rest[len(_PEE_TILE_TAG) + struct.calcsize(_PEE_TILE_FMT) + 4 * tiles["tile_crc32"].size:]
    md.update(_pee_aead_fields(rest))
    return md


def _pee_shape_check(bpp: int, width: int, height: int):
    if bpp not in (1, 2):
        raise ValueError(f"MED-PEE header: {bpp} bytes per pixel (1 or 2)")
    if width < 1 or height < 1:
        raise ValueError(f"MED-PEE header: width x height = {width} x {height}")


_PEE2_FMT = ">BBBBIIiiii"
_PEE2_PASS = ">iiiI"
PEE_SCHEME2 = 2


def create_pee2_header(codec: str, bytes_per_px: int, width: int, height: int, T: int, maxval: int, L: int,
                       status: int, passes: Sequence[Tuple[int, int, int, int]]) -> bytes:
    """Scheme-2 header; passes = 4 x (L_p, end_p, status_p, lm_blob_size_p)."""
    if len(passes) != 4:
        raise ValueError("scheme 2 has four passes")
    hdr = struct.pack(_PEE2_FMT, PEE_VERSION, CODEC_IDS.get(codec.lower(), 0), int(bytes_per_px), PEE_SCHEME2,
                      width, height, int(T), int(maxval), int(L), int(status))
    return hdr + b"".join(struct.pack(_PEE2_PASS, int(a), int(b), int(c), int(d)) for a, b, c, d in passes)


PEE_SCHEME_GATE = 3
_PEE_GATE_FMT = ">H"


def create_pee_gate_header(codec: str, bytes_per_px: int, width: int, height: int, T: int, L: int, end: int,
                           maxval: int, status: int, lm_blob_size: int, gate: int) -> bytes:
    """Header of a smoothness-gated scheme-1 file (scheme byte 3): scheme 1's fixed fields, then
    the gate as >H.  A reader that does not know the byte refuses the file, so a gated file is
    never decoded ungated."""
    if not 0 <= int(gate) <= 0xFFFF:
        raise ValueError(f"gate = {gate}: 0..65535")
    return struct.pack(_PEE_FMT, PEE_VERSION, CODEC_IDS.get(codec.lower(), 0), int(bytes_per_px), PEE_SCHEME_GATE,
                       width, height, int(T), int(L), int(end), int(maxval), int(status), int(lm_blob_size)) + \
        struct.pack(_PEE_GATE_FMT, int(gate))


def parse_pee_gate_bytes(data: bytes) -> Tuple[Dict, bytes, bytes]:
    """A gated version-16 STGC file (scheme byte 3) -> (side information with 'gate', lm_blob,
    stego bytes); 'cover_crc32' / 'payload_crc32' when the header carries the checksum extension."""
    if pee_scheme(data) == PEE_SCHEME_ROI:
        raise ValueError("a ROI-protected MED-PEE container (scheme byte 4): use parse_pee_roi_bytes")
    if pee_scheme(data) != PEE_SCHEME_GATE:
        raise ValueError("not a gated MED-PEE container (scheme byte 3)")
    n0 = struct.calcsize(_PEE_FMT)
    hdr, body = _pee_header(data, n0 + struct.calcsize(_PEE_GATE_FMT), "gated MED-PEE file")
    (_v, cid, bpp, _s, width, height, T, L, end, maxval, status, blob_size) = struct.unpack(_PEE_FMT, hdr[:n0])
    (gate,) = struct.unpack(_PEE_GATE_FMT, hdr[n0:n0 + struct.calcsize(_PEE_GATE_FMT)])
    _pee_shape_check(bpp, width, height)
    if blob_size > len(body):
        raise ValueError(f"truncated MED-PEE file: a location-map blob of {blob_size} bytes, {len(body)} left")
    md = {"version": PEE_VERSION, "scheme": PEE_SCHEME_GATE, "codec": CODEC_NAMES.get(cid, "raw" if cid == 0 else "unknown"),
          "bytes": bpp, "width": width, "height": height, "T": T, "L": L, "end": end, "maxval": maxval,
          "status": status, "gate": gate}
    md.update(_pee_ext_fields(hdr[n0 + struct.calcsize(_PEE_GATE_FMT):], width, height))
    return md, body[:blob_size], body[blob_size:]


PEE_SCHEME_ROI = 4
_PEE_ROI_FMT = ">HHHH"


def create_pee_roi_header(codec: str, bytes_per_px: int, width: int, height: int, T: int, L: int, end: int,
                          maxval: int, status: int, lm_blob_size: int, gate: int, roi) -> bytes:
    """Header of a ROI-protected scheme-1 file (scheme byte 4): scheme byte 3's fixed
    fields (scheme 1's, then the gate as >H -- 65535 when no gate was asked for) followed by the
    rectangle (y0, x0, y1, x1) as >HHHH.  The optional extensions follow as in every scheme.  A
    reader that knows scheme bytes 0, 2 and 3 refuses the file, so a protected file is never
    decoded without its rectangle."""
    if not 0 <= int(gate) <= 0xFFFF:
        raise ValueError(f"gate = {gate}: 0..65535")
    y0, x0, y1, x1 = (int(v) for v in roi)
    if not (0 <= y0 < y1 <= min(int(height), 0xFFFF) and 0 <= x0 < x1 <= min(int(width), 0xFFFF)):
        raise ValueError(f"roi = {(y0, x0, y1, x1)}: a non-empty rectangle inside {height} x {width} pixels (at most 65535 a side)")
    return struct.pack(_PEE_FMT, PEE_VERSION, CODEC_IDS.get(codec.lower(), 0), int(bytes_per_px), PEE_SCHEME_ROI,
                       width, height, int(T), int(L), int(end), int(maxval), int(status), int(lm_blob_size)) + \
        struct.pack(_PEE_GATE_FMT, int(gate)) + struct.pack(_PEE_ROI_FMT, y0, x0, y1, x1)


def parse_pee_roi_bytes(data: bytes) -> Tuple[Dict, bytes, bytes]:
    """A ROI-protected version-16 STGC file (scheme byte 4) -> (side information with 'gate' and
    'roi' = (y0, x0, y1, x1), lm_blob, stego bytes); 'cover_crc32' / 'payload_crc32' (and the tile
    fields) when the header carries the extensions.  ValueError for a header cut inside the
    rectangle, and for a rectangle that is empty or not inside the image."""
    if pee_scheme(data) != PEE_SCHEME_ROI:
        raise ValueError("not a ROI-protected MED-PEE container (scheme byte 4)")
    n0 = struct.calcsize(_PEE_FMT)
    n1 = n0 + struct.calcsize(_PEE_GATE_FMT)
    n2 = n1 + struct.calcsize(_PEE_ROI_FMT)
    hdr, body = _pee_header(data, n2, "ROI-protected MED-PEE file")
    (_v, cid, bpp, _s, width, height, T, L, end, maxval, status, blob_size) = struct.unpack(_PEE_FMT, hdr[:n0])
    (gate,) = struct.unpack(_PEE_GATE_FMT, hdr[n0:n1])
    y0, x0, y1, x1 = struct.unpack(_PEE_ROI_FMT, hdr[n1:n2])
    _pee_shape_check(bpp, width, height)
    if not (y0 < y1 <= height and x0 < x1 <= width):
        raise ValueError(f"MED-PEE header: the rectangle (y0, x0, y1, x1) = {(y0, x0, y1, x1)} is empty or not inside "
                         f"{height} x {width} pixels")
    if blob_size > len(body):
        raise ValueError(f"truncated MED-PEE file: a location-map blob of {blob_size} bytes, {len(body)} left")
    md = {"version": PEE_VERSION, "scheme": PEE_SCHEME_ROI, "codec": CODEC_NAMES.get(cid, "raw" if cid == 0 else "unknown"),
          "bytes": bpp, "width": width, "height": height, "T": T, "L": L, "end": end, "maxval": maxval,
          "status": status, "gate": gate, "roi": (y0, x0, y1, x1)}
    md.update(_pee_ext_fields(hdr[n2:], width, height))
    return md, body[:blob_size], body[blob_size:]


def pee_scheme(data: bytes) -> int:
    """1, 2, 3 or 4: the MED-PEE scheme of a version-16 STGC file (its scheme byte; 3 = scheme 1
    with a smoothness gate, 4 = scheme 1 with a protected rectangle and a gate)."""
    if data[:4] != MAGIC:
        raise ValueError("Arquivo inválido ou com assinatura incorreta.")   # codec.py:698
    if len(data) < 8:
        raise ValueError("truncated STGC file: no header length")
    (hlen,) = struct.unpack(">I", data[4:8])
    hdr = data[8:8 + hlen]
    if len(hdr) < 4 or hdr[0] != PEE_VERSION:
        raise ValueError("not a MED-PEE container (version 16)")
    if hdr[3] not in (0, PEE_SCHEME2, PEE_SCHEME_GATE, PEE_SCHEME_ROI):
        raise ValueError(f"unknown MED-PEE scheme byte {hdr[3]}")
    return 1 if hdr[3] == 0 else int(hdr[3])


def parse_pee2_bytes(data: bytes) -> Tuple[Dict, List[bytes], bytes]:
    """A scheme-2 version-16 STGC file -> (side information with 'passes', 4 lm blobs, stego bytes);
    'cover_crc32' / 'payload_crc32' when the header carries the checksum extension."""
    if pee_scheme(data) != 2:
        raise ValueError("not a scheme-2 MED-PEE container")
    n0 = struct.calcsize(_PEE2_FMT)
    hdr, body = _pee_header(data, n0 + 4 * struct.calcsize(_PEE2_PASS), "scheme-2 MED-PEE file")
    (_v, cid, bpp, _s, width, height, T, maxval, L, status) = struct.unpack(_PEE2_FMT, hdr[:n0])
    _pee_shape_check(bpp, width, height)
    passes, blobs, pos = [], [], 0
    for p in range(4):
        Lp, endp, stp, nb = struct.unpack(_PEE2_PASS, hdr[n0 + 16 * p: n0 + 16 * (p + 1)])
        if pos + nb > len(body):
            raise ValueError(f"truncated scheme-2 MED-PEE file: pass {p}'s location-map blob of {nb} bytes "
                             f"does not fit the {len(body) - pos} bytes left")
        passes.append({"L": Lp, "end": endp, "status": stp})
        blobs.append(body[pos:pos + nb])
        pos += nb
    md = {"version": PEE_VERSION, "scheme": 2, "codec": CODEC_NAMES.get(cid, "raw" if cid == 0 else "unknown"),
          "bytes": bpp, "width": width, "height": height, "T": T, "maxval": maxval, "L": L, "status": status,
          "passes": passes}
    md.update(_pee_ext_fields(hdr[n0 + 4 * struct.calcsize(_PEE2_PASS):], width, height))
    return md, blobs, body[pos:]


def parse_pee_bytes(data: bytes) -> Tuple[Dict, bytes, bytes]:
    """A version-16 STGC file of scheme 1 -> (side information, lm_blob, stego bytes);
    'cover_crc32' / 'payload_crc32' when the header carries the checksum extension."""
    scheme = pee_scheme(data)
    if scheme == PEE_SCHEME_ROI:
        raise ValueError("a ROI-protected MED-PEE container (scheme byte 4): use parse_pee_roi_bytes")
    if scheme == PEE_SCHEME_GATE:
        raise ValueError("a gated MED-PEE container (scheme byte 3): use parse_pee_gate_bytes")
    if scheme != 1:
        raise ValueError("a scheme-2 MED-PEE container: use parse_pee2_bytes")
    hdr, body = _pee_header(data, struct.calcsize(_PEE_FMT), "MED-PEE file")
    (_v, cid, bpp, _r, width, height, T, L, end, maxval, status, blob_size) = struct.unpack(
        _PEE_FMT, hdr[:struct.calcsize(_PEE_FMT)])
    _pee_shape_check(bpp, width, height)
    if blob_size > len(body):
        raise ValueError(f"truncated MED-PEE file: a location-map blob of {blob_size} bytes, {len(body)} left")
    md = {"version": PEE_VERSION, "codec": CODEC_NAMES.get(cid, "raw" if cid == 0 else "unknown"),
          "bytes": bpp, "width": width, "height": height, "T": T, "L": L, "end": end, "maxval": maxval,
          "status": status}
    md.update(_pee_ext_fields(hdr[struct.calcsize(_PEE_FMT):], width, height))
    return md, body[:blob_size], body[blob_size:]
